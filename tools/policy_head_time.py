"""What the policy's action head costs on one MI355X, each shape two ways in one process:

  rollout   40 960 rows (4096 envs x 10 agents), K = 25, under no_grad, with available_actions:
              new     gmpe.act_head: the head's Linear inside the sampling launch (gmpe_act_head, one launch)
              parent  F.linear + gmpe.sample_actions: a torch GEMM, then gmpe_act_sample — the path before the head was built
  train     512 000 rows, K = 25, forward + backward, each feeding the same gmpe.ppo_losses call and the backward of its actor_loss:
              new     gmpe.action_logits (gmpe_head_forward, one launch; gmpe_head_backward, three)
              parent  F.linear under torch's autograd (a GEMM forward, two GEMMs and a column sum backward)

The shipped head (tests/golden/policy_heads.npz, actor), features ~ N(0, 1). Timed with HIP events in alternating rounds of `iters` calls after a warm-up
of both paths at the timed shape (the comparison run and one untimed window each); median and range over the rounds. The results are compared before
anything is timed: the two paths' logits agree to float32 rounding (they are not the same bits: that is the point of the new one), the actions are
compared where the logits happen to agree in every bit of the row, and the gradients to 1e-4 of their largest element.

    python tools/policy_head_time.py [--rounds 7] [--out profiles/policy_head_time.json]
"""
import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

K, A = 25, 10
SHAPES = [dict(name="rollout", rows=40960, backward=False, iters=20), dict(name="train", rows=512000, backward=True, iters=5)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_head_time.json"))
    o = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F
    import gmpe
    import head_lib as HL
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    dev = "cuda"
    act = HL.act_layer(K, "actor", dev)
    lin = act.action_out.linear
    args = types.SimpleNamespace(use_valuenorm=False, use_popart=False)
    recs = []
    for s in SHAPES:
        rows, bwd, iters = s["rows"], s["backward"], s["iters"]
        rng = np.random.RandomState(rows)
        t = lambda a: torch.from_numpy(a).to(dev)
        feat = t(rng.randn(rows, 64).astype(np.float32))
        av = (rng.rand(rows, K) > 0.3).astype(np.float32)
        av[:, K // 2] = 1.0
        av = t(av)
        if not bwd:
            kw = dict(seed=1, num_agents=A, draw=0)
            out = {k: torch.empty((rows,), dtype=d, device=dev) for k, d in (("action_idx", torch.int32), ("action_log_probs", torch.float32))}

            def new():
                with torch.no_grad():
                    return gmpe.act_head(feat, act, av, out=out, **kw)

            def parent():
                with torch.no_grad():
                    return gmpe.sample_actions(F.linear(feat, lin.weight, lin.bias), av, out=out, **kw)
            with torch.no_grad():
                la, lb = gmpe.action_logits(feat, act), F.linear(feat, lin.weight, lin.bias)
            a = [x.clone() for x in new() if x is not None]
            b = [x.clone() for x in parent() if x is not None]
            samebits = (la.view(torch.int32) == lb.view(torch.int32)).all(dim=1)
            assert torch.equal(a[0][samebits], b[0][samebits]) and torch.equal(a[1].view(-1)[samebits], b[1].view(-1)[samebits])
            agree = float((a[0] == b[0]).float().mean())
            worst = float((la - lb).abs().max() / max(1.0, float(lb.abs().max())))
            assert worst < 1e-5 and agree > 0.999, (worst, agree)
            extra = dict(rows_with_equal_logit_bits=int(samebits.sum()), actions_agreeing=agree)
        else:
            r = np.random.RandomState(1)
            cols = dict(actions=t(r.randint(0, K, (rows, 1)).astype(np.int64)), value_preds=t(r.randn(rows, 1).astype(np.float32)),
                        returns=t(r.randn(rows, 1).astype(np.float32)), active_masks=t((r.rand(rows, 1) > 0.1).astype(np.float32)),
                        old_action_log_probs=t((-r.rand(rows, 1) * 3).astype(np.float32)), adv_targ=t(r.randn(rows, 1).astype(np.float32)), available_actions=av)
            values = t(r.randn(rows, 1).astype(np.float32))
            feat.requires_grad_(True)
            ws = torch.empty((gmpe.head_workspace_bytes(rows, K),), dtype=torch.uint8, device=dev)
            lws = torch.empty((gmpe.ppo_loss.workspace_bytes(rows),), dtype=torch.uint8, device=dev)

            def step(logits_of):
                feat.grad = lin.weight.grad = lin.bias.grad = None
                gmpe.ppo_losses(logits_of(), values, cols, args, workspace=lws).actor_loss.backward()
                return feat.grad, lin.weight.grad, lin.bias.grad
            new = lambda: step(lambda: gmpe.action_logits(feat, act, workspace=ws))
            parent = lambda: step(lambda: F.linear(feat, lin.weight, lin.bias))
            a = [x.clone() for x in new()]
            b = [x.clone() for x in parent()]
            worst = max(float((x - y).abs().max() / max(1e-30, float(y.abs().max()))) for x, y in zip(a, b))
            assert worst < 1e-4, worst
            extra = dict(workspace_bytes=int(ws.numel()))
        paths = {"new": new, "parent": parent}
        times = {k: [] for k in paths}
        for fn in paths.values():                       # one untimed window per path
            for _ in range(iters):
                fn()
        torch.cuda.synchronize()
        for _ in range(o.rounds):
            for k, fn in paths.items():                 # alternating rounds
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / iters)
        for k in paths:
            ts = sorted(times[k])
            rec = dict(shape=s["name"], rows=rows, K=K, backward=bwd, path=k, us_median=round(ts[len(ts) // 2], 1), us_min=round(ts[0], 1),
                       us_max=round(ts[-1], 1), max_rel_diff_new_vs_parent=worst, rounds=o.rounds, iters=iters,
                       note="rollout: act_head vs F.linear + sample_actions; train: action_logits vs F.linear, each + ppo_losses and actor_loss.backward()",
                       **extra)
            recs.append(rec)
            print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(o.out), exist_ok=True)
    with open(o.out, "w") as f:
        json.dump(recs, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
