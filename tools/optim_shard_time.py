"""What the sharded gradient clip and Adam step cost per call on ONE MI355X, next to the plain call of the same run:

  plain         gmpe.clip_and_step(optimizer, 10.0, parameters=..., workspace=...)                       two launches per 64 tensors
  shards_W      h = gmpe.clip_and_step_begin(...); all[0] = h.local; gmpe.clip_and_step_finish(h, all)   one launch before, two after, per 64 tensors

over the shipped actor's 52 tensors (the module of tests/test_gpu_policy.py with the weights of tests/golden/), every tensor with a gradient of
N(0, 0.01^2). The shards are emulated on one device: `all` is [W, n] with rows 1 .. W-1 zero, and the exchange is stood in for by one device copy of
`.local` into row 0 (included in both numbers) — so the sum is the gradient itself, the clip multiplies by 1 and the gradients keep their bits from call
to call, while k_opt_reduce still reads all W rows. The collective itself, and anything across several GPUs, is NOT measured here.

device_us / host_us as in tools/optim_step_time.py: HIP events around `iters` calls enqueued behind a sleeping kernel; a host clock around `iters` calls
ending in one synchronise, minus device_us. Alternating rounds after a warm-up window of each path; median and range. One run on one box.

    python tools/optim_shard_time.py [--worlds 2 8] [--rounds 7] [--iters 50] [--out profiles/optim_shard_time.json]
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
# run as a script, python puts tools/ first on the path, where profile.py would shadow the standard library's `profile` that torch's optimisers import
sys.path[:] = [p for p in sys.path if os.path.abspath(p or ".") != HERE]
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MAX_NORM, LR, EPS = 10.0, 5e-4, 1e-5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", type=int, nargs="+", default=[2, 8])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_shard_time.json"))
    o = ap.parse_args()
    import copy
    import torch
    import gmpe
    import gnn_lib as G
    from test_gpu_policy import OBS, _Net
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    dev = "cuda"
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    e0.record()
    torch.cuda._sleep(20000000)
    e1.record()
    torch.cuda.synchronize()
    cycles_per_us = 20000000 / (e0.elapsed_time(e1) * 1e3)
    net = _Net(G.ACTOR, OBS, "act")
    gen = torch.Generator().manual_seed(5)
    grads = [torch.randn(p.shape, generator=gen) * 0.01 for p in net.parameters()]
    n = sum(g.numel() for g in grads)

    def build():
        m = copy.deepcopy(net).to(dev)
        ps = list(m.parameters())
        for p, g in zip(ps, grads):
            p.grad = g.to(dev)
        opt = torch.optim.Adam(ps, lr=LR, eps=EPS)
        return ps, opt, torch.empty((gmpe.optim.workspace_bytes(opt),), dtype=torch.uint8, device=dev)

    paths, state = {}, {}
    ps, opt, ws = build()
    paths["plain"] = lambda ps=ps, opt=opt, ws=ws: gmpe.clip_and_step(opt, MAX_NORM, parameters=ps, workspace=ws)
    state["plain"] = ps
    for W in o.worlds:
        ps, opt, ws = build()
        all_ = torch.zeros((W, n), dtype=torch.float32, device=dev)

        def sharded(ps=ps, opt=opt, ws=ws, all_=all_):
            h = gmpe.clip_and_step_begin(opt, MAX_NORM, parameters=ps, workspace=ws)
            all_[0].copy_(h.local)
            return gmpe.clip_and_step_finish(h, all_)
        paths["shards_%d" % W], state["shards_%d" % W] = sharded, ps
    # equal start, three steps each: the sharded paths give the plain call's bits before anything is timed
    norms = {k: [float(fn()) for _ in range(3)][-1] for k, fn in paths.items()}
    assert all(v == norms["plain"] for v in norms.values()) and norms["plain"] < MAX_NORM, norms
    assert all(torch.equal(a, b) for k in paths for a, b in zip(state[k], state["plain"]))
    for fn in paths.values():                           # one untimed window per path
        for _ in range(o.iters):
            fn()
    torch.cuda.synchronize()
    wall, device = {k: [] for k in paths}, {k: [] for k in paths}
    for _ in range(o.rounds):
        for k, fn in paths.items():                     # alternating rounds
            t0 = time.perf_counter()
            for _ in range(o.iters):
                fn()
            torch.cuda.synchronize()
            w = (time.perf_counter() - t0) * 1e6
            wall[k].append(w / o.iters)
            torch.cuda._sleep(int(cycles_per_us * w * 1.5))             # the host runs ahead of the device: the calls wait in the queue
            e0.record()
            for _ in range(o.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            device[k].append(e0.elapsed_time(e1) * 1e3 / o.iters)
    med = lambda xs: sorted(xs)[len(xs) // 2]
    recs = []
    for k in paths:
        host = [w - d for w, d in zip(wall[k], device[k])]
        rec = dict(network="actor", tensors=len(grads), elements=n, path=k, world=int(k.split("_")[1]) if "_" in k else None,
                   gathered_bytes=4 * n * int(k.split("_")[1]) if "_" in k else 0, device_us_median=round(med(device[k]), 1),
                   device_us_min=round(min(device[k]), 1), device_us_max=round(max(device[k]), 1), host_us_median=round(med(host), 1),
                   host_us_min=round(min(host), 1), host_us_max=round(max(host), 1), wall_us_median=round(med(wall[k]), 1), rounds=o.rounds, iters=o.iters,
                   note="per call; shards emulated on one device, the exchange stood in for by one device copy of .local (included); the collective and "
                        "any multi-GPU figure are unmeasured; device: events behind a sleeping kernel; host: wall - device; one run on one box")
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(o.out), exist_ok=True)
    with open(o.out, "w") as f:
        json.dump(recs, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
