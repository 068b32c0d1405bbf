"""What drawing PPO minibatches from a rollout costs on one MI355X (GraphReplayBuffer.feed_forward_generator / recurrent_generator), three ways, at c3 and c4
rollout shapes (T = 25; recurrent with data_chunk_length 10 and the reference's --auto_mini_batch_size --target_mini_batch_size 8192 minibatch count,
onpolicy/config.py:472-481; feed-forward with the same count):

  fused   gmpe.minibatch.Gather: one gmpe_minibatch_gather call per minibatch (gmpe_minibatch.hip), for each storage form of the rollout
          (rows + materialised adjacency [c3 only], rows + compact adjacency, entity table + no adjacency)
  torch   advanced indexing of the materialised [T+1, N, A, ...] arrays on the device, field by field (c3 only: c4's materialised adjacency is over 100 GB)
  numpy   the reference's host gather of one minibatch from host arrays (a subset of the envs, same minibatch size) + H2D of the result; the D2H of the
          rollout that would come first is NOT included: a lower bound

fused and torch are timed with HIP events over `--batches` consecutive minibatches of one epoch after a warm-up; numpy with a host clock. Bytes = what one
minibatch writes (the inputs are random: the gather does not look at values). GB/s of written bytes against the store ceilings in profiles/r04_fillbw.json.
The fused minibatches are checked against the torch ones (c3) before anything is timed.

    python tools/minibatch_bw.py [--batches 40] [--numpy-batches 3]      # one JSON line per (shape, mode, path) + a summary table
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"c3": (25, 4096, 10), "c4": (25, 8192, 32)}
L, TARGET, R, H, NUMPY_ENVS = 10, 8192, 1, 64, 512


def arrays_for(torch, cfg, T, N, form, g):
    A, E, F, D, W = cfg.num_agents, cfg.num_entities, cfg.node_feats, cfg.obs_dim, cfg.entity_table_width
    dev = "cuda"
    r = lambda *s: torch.rand(s, generator=g, device=dev)
    a = dict(obs=r(T + 1, N, A, D), agent_id=torch.randint(0, A, (T + 1, N, A, 1), generator=g, device=dev, dtype=torch.int32),
             masks=r(T + 1, N, A, 1), active_masks=r(T + 1, N, A, 1), value_preds=r(T + 1, N, A, 1), returns=r(T + 1, N, A, 1),
             available_actions=r(T + 1, N, A, cfg.n_actions), advantages=r(T, N, A, 1), rnn_states=r(T + 1, N, A, R, H), rnn_states_critic=r(T + 1, N, A, R, H),
             actions=r(T, N, A, 1), action_log_probs=r(T, N, A, 1))
    if form == "table":
        tab = torch.rand((T + 1, N, W), generator=g, device=dev, dtype=torch.float64) * 10
        tab[..., W - (E + 31) // 32:] = 0                                # no masked entity
        a["entity_table"] = tab
    else:
        a["node_obs"] = r(T + 1, N, A, E, F)
        a["adj"] = r(T + 1, N, E, E) if form == "compact" else r(T + 1, N, A, E, E)
    return a


def torch_batch(_, a, t, n, ai, ht, hn, ha):
    """advanced indexing of the materialised arrays at samples (t, n, a); rnn rows at (ht, hn, ha)"""
    T1, N, A, D = a["obs"].shape
    o = {k: a[k][t, n, ai] for k in ("obs", "node_obs", "adj", "agent_id", "actions", "value_preds", "returns", "masks", "active_masks", "action_log_probs",
                                     "advantages", "available_actions")}
    o["share_obs"] = a["obs"][t, n].reshape(len(t), A * D)
    o["share_agent_id"] = a["agent_id"][t, n].reshape(len(t), A)
    for k in ("rnn_states", "rnn_states_critic"):
        o[k] = a[k][ht, hn, ha]
    return o


def samples(xp, perm, off, rows, T, N, A, rec):
    """(t, n, a) of the output rows and of the rnn rows (chunk heads) of one minibatch; xp: torch (device permutation) or numpy (host)"""
    if not rec:
        j = perm[off:off + rows]
        s = (j // (N * A), (j // A) % N, j % A)
        return s, s
    c = perm[off:off + rows]
    ar = xp.arange(L, device=c.device) if xp is not np else np.arange(L)
    f = (c[None, :] * L + ar[:, None]).reshape(-1)
    dec = lambda f: (f % T, f // (A * T), (f // T) % A)
    return dec(f), dec(c * L)


def timed(torch, fn, batches, warm=3):
    for i in range(warm):
        fn(i)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(batches):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / batches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=40)
    ap.add_argument("--numpy-batches", type=int, default=3)
    ap.add_argument("--shapes", default="c3,c4")
    args = ap.parse_args()
    import torch
    import gmpe
    from gmpe.minibatch import Gather, recurrent_sizes
    fill = json.load(open(os.path.join(ROOT, "profiles", "r04_fillbw.json")))["fill_GBps"]
    rows_out = []
    for shape in args.shapes.split(","):
        T, N, A = SHAPES[shape]
        cfg = gmpe.make_config(num_envs=N, num_agents=A, episode_length=T)
        nmb = N * T * A // TARGET
        g = torch.Generator(device="cuda"); g.manual_seed(0)
        forms = ("materialised", "compact", "table") if shape == "c3" else ("compact", "table")
        for form in forms:
            a = arrays_for(torch, cfg, T, N, form, g)
            for rec in (False, True):
                gat = Gather(cfg, a, L if rec else None, use_centralized_V=True)
                n = gat.num_units
                perm = torch.randperm(n, device="cuda", generator=g)
                per = recurrent_sizes(T, N, A, nmb, L)[1] if rec else n // nmb
                nb = min(args.batches, nmb - 3)
                out_bytes = gat.out_bytes(per)
                rec_row = dict(shape=shape, T=T, N=N, A=A, E=cfg.num_entities, mode="recurrent" if rec else "feed_forward", num_mini_batch=nmb,
                               rows=per * (L if rec else 1), bytes_per_minibatch=out_bytes, bytes_per_sample=round(out_bytes / (per * (L if rec else 1)), 1))
                if form == "materialised":                                # check the fused minibatch against torch indexing first
                    s, hs = samples(torch, perm, 0, per, T, N, A, rec)
                    want, got = torch_batch(torch, a, *s, *hs), gat(perm, 0, per)
                    assert all(torch.equal(got[k], want[k]) for k in want), "fused != torch indexing"
                    us = timed(torch, lambda i: torch_batch(torch, a, *[x for p in samples(torch, perm, i * per, per, T, N, A, rec) for x in p]), nb)
                    rows_out.append(dict(rec_row, path="torch", form=form, us=round(us, 1), GBps=round(out_bytes / us / 1e3, 1)))
                us = timed(torch, lambda i: gat(perm, i * per, per), nb)
                rows_out.append(dict(rec_row, path="fused", form=form, us=round(us, 1), GBps=round(out_bytes / us / 1e3, 1),
                                     frac_of_fill_98MB_cache=round(out_bytes / us / 1e3 / fill["98MB"], 3),
                                     frac_of_fill_2p5GB_dram=round(out_bytes / us / 1e3 / fill["2.5GB"], 3)))
                print(json.dumps(rows_out[-1]), flush=True)
                if form == "compact" and shape == "c3":                   # host path on a subset of the envs (materialised per-agent arrays, as the reference keeps them)
                    Ns = NUMPY_ENVS
                    h = {k: v[:, :Ns].cpu().numpy() for k, v in a.items()}
                    h["adj"] = np.repeat(h["adj"][:, :, None], A, axis=2)
                    hp = np.random.RandomState(0).permutation(T * Ns * A // (L if rec else 1))
                    def np_batch(i):
                        s, hs = samples(np, hp, i * per, per, T, Ns, A, rec)
                        o = torch_batch(np, h, *s, *hs)
                        return {k: torch.from_numpy(np.ascontiguousarray(v)).to("cuda", non_blocking=False) for k, v in o.items()}
                    np_batch(0)
                    t0 = time.perf_counter()
                    for i in range(args.numpy_batches):
                        np_batch(i)
                    torch.cuda.synchronize()
                    us = (time.perf_counter() - t0) * 1e6 / args.numpy_batches
                    rows_out.append(dict(rec_row, path="numpy", form="host subset %d envs" % Ns, us=round(us, 1), GBps=round(out_bytes / us / 1e3, 2)))
            del a
            torch.cuda.empty_cache()
    print()
    for r in rows_out:
        if r["path"] != "fused":
            print(json.dumps(r))
    print("%-5s %-12s %-6s %-22s %10s %8s %9s" % ("shape", "mode", "path", "form", "us/minib", "GB/s", "KB/sample"))
    for r in rows_out:
        print("%-5s %-12s %-6s %-22s %10.1f %8.1f %9.2f" % (r["shape"], r["mode"], r["path"], r["form"], r["us"], r["GBps"], r["bytes_per_sample"] / 1e3))


if __name__ == "__main__":
    main()
