"""What the learner-side stage after a rollout costs on one MI355X: returns (GAE, ValueNorm-denormalised: the shipped runner's flags) + raw and
normalised advantages (GraphReplayBuffer.compute_returns + the head of GR_MAPPO.train), three ways, at c3 and c4 rollout shapes (T = 25):

  fused   gmpe.engine.compute_returns: one returns launch + the two-launch masked mean / std normalisation (gmpe_returns.hip)
  torch   the same math as a loop of torch ops on the device (what a device runner would write without the kernels)
  numpy   the reference's path: D2H of rewards / masks / value_preds / next_value / active_masks, the float32 NumPy loop of compute_returns and
          train's nanmean / nanstd lines, H2D of returns and advantages (ValueNorm.denormalize's torch round trip per step is NOT included: a lower bound)

fused and torch are timed with HIP events over `--reps` back-to-back calls after a warm-up; numpy with a host clock around synchronised calls.
Bytes = what the fused path moves (reads: rewards, masks[1:], value_preds[:-1], active_masks[:-1], next_value; writes: returns[:-1],
value_preds[T], the raw advantages; the normalisation reads and rewrites them), against the store ceilings recorded in profiles/r04_fillbw.json.
Results are checked: fused returns == NumPy returns bit for bit, normalised advantages within 1e-4 of NumPy's float32 nanmean / nanstd.

    python tools/returns_bw.py [--reps 200] [--numpy-reps 5]        # one JSON line per (shape, path) + a summary table
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
GAMMA, LAM = 0.99, 0.95


def numpy_path(torch, d):
    """D2H, the reference's float32 loop (GAE, valuenorm branch of graph_buffer.py:341-352) and train's lines (graph_mappo.py:294-304), H2D."""
    rew, masks, vp, nv, am = (t.cpu().numpy() for t in (d["rewards"], d["masks"], d["value_preds"], d["next_value"], d["active_masks"]))
    mean, std = d["mean"].cpu().numpy(), d["std"].cpu().numpy()
    dn = lambda x: x * std + mean
    ret = np.zeros_like(vp)
    vp[-1] = nv
    gae = 0
    for step in reversed(range(rew.shape[0])):
        delta = rew[step] + GAMMA * dn(vp[step + 1]) * masks[step + 1] - dn(vp[step])
        gae = delta + GAMMA * LAM * masks[step + 1] * gae
        ret[step] = gae + dn(vp[step])
    adv = ret[:-1] - dn(vp[:-1])
    a2 = adv.copy()
    a2[am[:-1] == 0.0] = np.nan
    adv = (adv - np.nanmean(a2)) / (np.nanstd(a2) + 1e-5)
    return torch.as_tensor(ret, device="cuda"), torch.as_tensor(adv, device="cuda")


def torch_path(torch, d, out):
    rew, masks, vp, nv, am = d["rewards"], d["masks"], d["value_preds"], d["next_value"], d["active_masks"]
    mean, std = d["mean"], d["std"]
    ret, adv = out["returns"], out["advantages"]
    vp[-1].copy_(nv)
    dv = vp * std + mean
    gae = torch.zeros_like(nv)
    gl = float(np.float32(GAMMA * LAM))
    for step in reversed(range(rew.shape[0])):
        delta = rew[step] + GAMMA * dv[step + 1] * masks[step + 1] - dv[step]
        gae = delta + gl * masks[step + 1] * gae
        ret[step] = gae + dv[step]
    torch.sub(ret[:-1], dv[:-1], out=adv)
    keep = (am[:-1] != 0).double()                               # masked sums, no boolean indexing: no host sync
    a = adv.double()
    n = keep.sum()
    m = (a * keep).sum() / n
    s = (((a - m) * keep) ** 2).sum().div(n).sqrt()
    adv.sub_(m.float()).div_(s.float() + 1e-5)


def fused_path(torch, gmpe, d, out, ws):
    gmpe.engine.compute_returns(d["rewards"], d["masks"], d["value_preds"], out["returns"], d["next_value"], gamma=GAMMA, gae_lambda=LAM,
                                use_gae=True, denorm=(d["mean"], d["std"]), advantages=out["advantages"], active_masks=d["active_masks"],
                                normalized=out["advantages"], workspace=ws)


def events_us(torch, fn, reps, warm=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--numpy-reps", type=int, default=5)
    ap.add_argument("--shapes", default="c3,c4")
    args = ap.parse_args()
    import torch
    import gmpe
    if not torch.cuda.is_available():
        sys.exit("returns_bw: no GPU visible (this tool measures the MI355X; there is no CPU number to report)")
    fill = json.load(open(os.path.join(ROOT, "profiles", "r04_fillbw.json")))["fill_GBps"]
    rows = []
    for tag in args.shapes.split(","):
        T, N, A = SHAPES[tag]
        L = N * A
        rng = np.random.RandomState(0)
        f = lambda *s: torch.as_tensor(rng.randn(*s).astype(np.float32), device="cuda")
        m = lambda *s, p=0.1: torch.as_tensor((rng.rand(*s) > p).astype(np.float32), device="cuda")
        d = dict(rewards=f(T, N, A, 1), masks=m(T + 1, N, A, 1), value_preds=f(T + 1, N, A, 1), next_value=f(N, A, 1), active_masks=m(T + 1, N, A, 1, p=0.2),
                 mean=torch.tensor([0.4], device="cuda"), std=torch.tensor([1.7], device="cuda"))
        out = dict(returns=torch.zeros(T + 1, N, A, 1, device="cuda"), advantages=torch.zeros(T, N, A, 1, device="cuda"))
        ws = torch.empty(gmpe.engine.returns_workspace_bytes(L), dtype=torch.uint8, device="cuda")
        nbytes = 4 * L * (7 * T + 2)     # reads 4T + 1, writes T + 1, normalisation reads and writes T each
        # correctness first: fused vs the NumPy path on the same inputs
        fused_path(torch, gmpe, d, out, ws)
        torch.cuda.synchronize()
        ret_np, adv_np = numpy_path(torch, d)
        same_ret = bool(torch.equal(out["returns"][:-1], ret_np[:-1]))
        adv_err = float((out["advantages"] - adv_np).abs().max())
        tout = dict(returns=torch.zeros_like(out["returns"]), advantages=torch.zeros_like(out["advantages"]))
        torch_path(torch, d, tout)
        torch_err = float((tout["advantages"] - adv_np).abs().max())
        res = {"fused": events_us(torch, lambda: fused_path(torch, gmpe, d, out, ws), args.reps),
               "torch": events_us(torch, lambda: torch_path(torch, d, tout), max(args.reps // 10, 5), warm=3)}
        numpy_path(torch, d)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.numpy_reps):
            numpy_path(torch, d)
            torch.cuda.synchronize()
        res["numpy"] = (time.perf_counter() - t0) * 1e6 / args.numpy_reps
        for path, us in res.items():
            row = {"shape": tag, "T": T, "N": N, "A": A, "path": path, "us": round(us, 2), "fused_min_bytes": nbytes,
                   "GBps_of_fused_bytes": round(nbytes / us / 1e3, 1),
                   "frac_of_fill_98MB_cache": round(nbytes / us / 1e3 / fill["98MB"], 3), "frac_of_fill_2p5GB_dram": round(nbytes / us / 1e3 / fill["2.5GB"], 3),
                   "fused_returns_bitwise_eq_numpy": same_ret, "fused_adv_maxerr_vs_numpy": adv_err, "torch_adv_maxerr_vs_numpy": torch_err}
            rows.append(row)
            print(json.dumps(row), flush=True)
    print("\nshape  path    us        GB/s   frac(98MB fill)")
    for r in rows:
        print("%-6s %-6s %9.1f %8.1f  %.3f" % (r["shape"], r["path"], r["us"], r["GBps_of_fused_bytes"], r["frac_of_fill_98MB_cache"]))
    bad = [r for r in rows if not r["fused_returns_bitwise_eq_numpy"] or r["fused_adv_maxerr_vs_numpy"] > 1e-4]
    if bad:
        sys.exit("returns_bw: fused results differ from the NumPy path")


if __name__ == "__main__":
    main()
