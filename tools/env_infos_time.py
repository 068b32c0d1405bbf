"""What run()'s log and eval bookkeeping costs on one MI355X, each two ways in one process, at 64 envs x 3 agents and at 4096 x 10:

  env_infos   new     gmpe.env_infos(info): one launch of gmpe_env_infos, the [A, 18] float64 means left on the device
              parent  the only route there was to the same numbers: info.cpu() and the NumPy restatement of process_infos + log_env
                      (tests/infos_lib.py info_means, the adds vectorised over the A * 18 columns — faster than the reference's dict loop)
  eval_step   new     gmpe.infos.eval_step: one launch of gmpe_eval_step behind an env step (reward sums, per-env masks, zeroed RNN rows)
              parent  the same bookkeeping in torch ops: done.all(dim=1), two masked writes, an add

One repetition = ITERS calls; wall time (perf_counter around the calls and a synchronize) and event time (HIP events around the calls) per call.
Three repetitions each, alternating, after one untimed repetition of both paths; every figure of every repetition is written, with its median.

    python tools/env_infos_time.py [--out profiles/env_infos_time.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REPS, T, DT = 3, 25, 0.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "env_infos_time.json"))
    o = ap.parse_args()
    import numpy as np
    import torch
    import gmpe
    import infos_lib as IL
    from gmpe import infos
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    dev = "cuda:0"
    recs = []

    def timed(fn):
        """(wall, event) microseconds of one call of fn"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return (time.perf_counter() - w0) * 1e6, e0.elapsed_time(e1) * 1e3

    def measure(paths, per, what, **extra):
        for fn in paths.values():
            fn()
        times = {k: [] for k in paths}
        for _ in range(REPS):
            for k, fn in paths.items():
                times[k].append(timed(fn))
        for k in paths:
            wall, event = sorted(w / per[k] for w, _ in times[k]), sorted(e / per[k] for _, e in times[k])
            rec = dict(what=what, path=k, wall_us=[round(x, 1) for x in wall], event_us=[round(x, 1) for x in event], wall_us_median=round(wall[1], 1),
                       event_us_median=round(event[1], 1), repetitions=REPS, calls_per_repetition=per[k], **extra)
            recs.append(rec)
            print(json.dumps(rec), flush=True)

    for N, A in ((64, 3), (4096, 10)):
        rng = np.random.RandomState(N)
        host = (rng.standard_normal((N, A, 18)) * np.exp(rng.uniform(-6.0, 6.0, (N, A, 18)))).astype(np.float32)
        host[..., 2] = np.where(rng.rand(N, A) < 0.3, -1.0, np.abs(host[..., 2]) + 0.1)
        info = torch.from_numpy(host).to(dev)
        out = torch.empty((A, 18), dtype=torch.float64, device=dev)
        per = {"new": 50, "parent": 3}

        def new():
            for _ in range(per["new"]):
                infos.env_infos(info, episode_length=T, dt=DT, out=out)

        def parent():
            for _ in range(per["parent"]):
                IL.info_means(info.cpu().numpy(), T, DT)
        got = infos.env_infos(info, episode_length=T, dt=DT)
        want = IL.env_infos(host, T, DT)
        assert list(got) == list(want) and IL.same_bits(np.array([v.item() for v in got.values()]), np.array(list(want.values())))
        measure({"new": new, "parent": parent}, per, "env_infos", num_envs=N, num_agents=A,
                note="per call; new: gmpe.env_infos (values stay on the device), parent: info.cpu() + the NumPy restatement (values on the host)")

        # ------------------------------------------------------------------ the eval step's bookkeeping
        R, H = 1, 64
        reward = torch.from_numpy(rng.standard_normal((N, A)).astype(np.float32)).to(dev)
        done = torch.from_numpy((rng.rand(N, A) < 0.5).astype(np.uint8)).to(dev)
        done[::5] = 1                                                               # a fifth of the envs finish
        state = [dict(sums=torch.zeros((N, A), dtype=torch.float64, device=dev), masks=torch.ones((N, A, 1), device=dev),
                      rnn=torch.ones((N, A, R, H), device=dev)) for _ in range(2)]
        per = {"new": 50, "parent": 50}

        def new(s=state[0]):
            for _ in range(per["new"]):
                infos.eval_step(reward, done, s["sums"], s["masks"], s["rnn"])

        def parent(s=state[1]):
            for _ in range(per["parent"]):
                all_done = done.bool().all(dim=1)
                s["rnn"].masked_fill_(all_done.view(N, 1, 1, 1), 0.0)
                s["masks"].fill_(1.0).masked_fill_(all_done.view(N, 1, 1), 0.0)
                s["sums"].add_(reward.double())
        new(), parent()
        assert all(torch.equal(state[0][k], state[1][k]) for k in state[0])
        measure({"new": new, "parent": parent}, per, "eval_step", num_envs=N, num_agents=A, rnn_row=R * H,
                note="per call; new: one launch of gmpe_eval_step, parent: done.all(dim=1), two masked writes, an add in torch ops")
    os.makedirs(os.path.dirname(o.out), exist_ok=True)
    with open(o.out, "w") as f:
        json.dump(recs, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
