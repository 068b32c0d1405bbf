"""What the gradient clip and the Adam step of one network cost per call on one MI355X, three ways in one process:

  gmpe          gmpe.clip_and_step(optimizer, 10.0, parameters=..., workspace=...)      two launches per 64 tensors, no wait
  torch         nn.utils.clip_grad_norm_(parameters, 10.0); optimizer.step()            torch's default (foreach) implementation
  torch_fused   the same with torch.optim.Adam(..., fused=True), where torch offers it

over the parameter sets of the shipped actor and critic (the modules of tests/test_gpu_policy.py with the weights of tests/golden/), every tensor with
a gradient of N(0, 0.01^2) — their norm stays under 10, so the clip multiplies by 1 and the gradients keep their bits from call to call.

Two numbers per path, per call:
  device_us   HIP events around `iters` calls that were enqueued behind a sleeping kernel, so the device finds them queued and the events see its time
              alone;
  host_us     a host clock around `iters` calls that ends in one synchronise, minus device_us: what the host adds — Python, launches, waits. This is
              the side the call is about.
The three paths start from equal state and their parameters are compared after three steps before anything is timed. Alternating rounds after a
warm-up window of each path; median and range over the rounds. One run on one box: the spread between boxes is not in it.

    python tools/optim_step_time.py [--rounds 7] [--iters 50] [--out profiles/optim_step_time.json]
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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_step_time.json"))
    o = ap.parse_args()
    import copy
    import torch
    import gmpe
    import gnn_lib as G
    from test_gpu_policy import OBS, _Net
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    dev = "cuda"
    # cycles of torch.cuda._sleep per microsecond, measured
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    e0.record()
    torch.cuda._sleep(20000000)
    e1.record()
    torch.cuda.synchronize()
    cycles_per_us = 20000000 / (e0.elapsed_time(e1) * 1e3)
    recs = []
    for name, net in (("actor", _Net(G.ACTOR, OBS, "act")), ("critic", _Net(G.CRITIC, OBS, "v_out", seed=12))):
        gen = torch.Generator().manual_seed(5)
        grads = [torch.randn(p.shape, generator=gen) * 0.01 for p in net.parameters()]

        def build(**kw):
            m = copy.deepcopy(net).to(dev)
            ps = list(m.parameters())
            for p, g in zip(ps, grads):
                p.grad = g.to(dev)
            return ps, torch.optim.Adam(ps, lr=LR, eps=EPS, **kw)

        paths, state = {}, {}
        ps, opt = build()
        ws = torch.empty((gmpe.optim.workspace_bytes(opt),), dtype=torch.uint8, device=dev)
        paths["gmpe"] = lambda ps=ps, opt=opt: gmpe.clip_and_step(opt, MAX_NORM, parameters=ps, workspace=ws)
        state["gmpe"] = ps

        def torch_path(ps, opt):
            def run():
                norm = torch.nn.utils.clip_grad_norm_(ps, MAX_NORM)
                opt.step()
                return norm
            return run
        ps, opt = build()
        paths["torch"], state["torch"] = torch_path(ps, opt), ps
        try:
            ps, opt = build(fused=True)
            paths["torch_fused"], state["torch_fused"] = torch_path(ps, opt), ps
        except (RuntimeError, ValueError, TypeError) as e:
            print("fused Adam is not offered here: %s" % e, flush=True)
        # equal start, three steps each: the parameters agree before anything is timed
        norms = {k: [float(fn()) for _ in range(3)][-1] for k, fn in paths.items()}
        worst = {k: max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(state[k], state["torch"])) for k in paths}
        assert all(w < 1e-5 for w in worst.values()) and all(abs(n - norms["torch"]) <= 1e-6 * norms["torch"] for n in norms.values()), (worst, norms)
        assert norms["torch"] < MAX_NORM
        n_tensors, n_elements = len(grads), sum(g.numel() for g in grads)
        for fn in paths.values():                       # one untimed window per path
            for _ in range(o.iters):
                fn()
        torch.cuda.synchronize()
        wall, device = {k: [] for k in paths}, {k: [] for k in paths}
        for _ in range(o.rounds):
            for k, fn in paths.items():                 # alternating rounds
                t0 = time.perf_counter()
                for _ in range(o.iters):
                    fn()
                torch.cuda.synchronize()
                w = (time.perf_counter() - t0) * 1e6
                wall[k].append(w / o.iters)
                torch.cuda._sleep(int(cycles_per_us * w * 1.5))         # the host runs ahead of the device: the calls wait in the queue
                e0.record()
                for _ in range(o.iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                device[k].append(e0.elapsed_time(e1) * 1e3 / o.iters)
        med = lambda xs: sorted(xs)[len(xs) // 2]
        for k in paths:
            host = [w - d for w, d in zip(wall[k], device[k])]
            rec = dict(network=name, tensors=n_tensors, elements=n_elements, path=k, device_us_median=round(med(device[k]), 1),
                       device_us_min=round(min(device[k]), 1), device_us_max=round(max(device[k]), 1), host_us_median=round(med(host), 1),
                       host_us_min=round(min(host), 1), host_us_max=round(max(host), 1), wall_us_median=round(med(wall[k]), 1),
                       max_rel_param_diff_vs_torch=worst[k], rounds=o.rounds, iters=o.iters,
                       note="per call of clip + Adam step; device: events behind a sleeping kernel; host: wall - device; one run on one box")
            recs.append(rec)
            print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(o.out), exist_ok=True)
    with open(o.out, "w") as f:
        json.dump(recs, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
