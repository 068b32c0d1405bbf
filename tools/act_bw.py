"""What the rollout half of the action head costs on one MI355X per act, two ways:

  fused   gmpe.sample_actions: one gmpe_act_sample launch — masks the logits from the previous step's dones, draws, writes the int32 action the engine
          takes, the float32 action and the log-prob into preallocated outputs
  torch   the sequence it replaces, as device torch ops: the stop-action rows (gmpe_available_actions_from_dones, [rows, K] floats), the masked fill,
          torch.distributions.Categorical (logsumexp, softmax), sample (multinomial), log_prob (gather), .to(int32), .float()

Shapes: rows = 4096 * 10, K = 5 and 25 (the bench shape's N * A). Timed with HIP events in alternating rounds after a warm-up; median and range over
the rounds. The kernel is small and launch-bound; what it gains in a real step, next to the policy's forward pass, is not measured here.
The fused actions are checked before anything is timed: available, and their log-probs equal to torch's for the same actions to float32 rounding.

    python tools/act_bw.py [--rounds 9] [--iters 50]      # one JSON line per (shape, path) + a summary table
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, A = 4096, 10
SHAPES = [(N * A, 5), (N * A, 25)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=50)
    o = ap.parse_args()
    import torch
    import gmpe
    from gmpe.engine import available_actions_from_dones
    rows_out = []
    for B, K in SHAPES:
        g = torch.Generator(device="cuda")
        g.manual_seed(B + K)
        logits = torch.randn((B, K), generator=g, device="cuda") * 2.0
        dones = (torch.rand((2, N, A), generator=g, device="cuda") < 0.3).to(torch.uint8)
        avail = torch.ones((2, N, A, K), device="cuda")
        out = dict(action_idx=torch.zeros(B, dtype=torch.int32, device="cuda"), actions_f32=torch.zeros(B, 1, device="cuda"),
                   action_log_probs=torch.zeros(B, 1, device="cuda"))
        state = dict(draw=0)

        def fused():
            gmpe.sample_actions(logits, dones_prev=dones[0], seed=1, num_agents=A, draw=state["draw"], out=out)
            state["draw"] += 1
            return out["action_idx"], out["actions_f32"], out["action_log_probs"]

        def stock():
            available_actions_from_dones(dones, avail, first=1, count=1)           # position 1 reads dones slot 0
            x = logits.clone()
            x[avail[1].view(B, K) == 0] = torch.finfo(torch.float32).min
            dist = torch.distributions.Categorical(logits=x, validate_args=False)
            a = dist.sample().unsqueeze(-1)
            lp = dist.log_prob(a.squeeze(-1)).unsqueeze(-1)
            return a.view(N, A).to(torch.int32), a.float(), lp
        paths = {"fused": fused, "torch": stock}
        idx, af, lp = (t.clone() for t in fused())
        stock()                                                        # fills the availability rows the fused path never writes
        av = avail[1].view(B, K)
        assert bool((av.gather(1, idx.long().view(B, 1)) == 1).all()) and bool((af.view(-1) == idx.float()).all())
        x = logits.clone()
        x[av == 0] = torch.finfo(torch.float32).min
        want = torch.distributions.Categorical(logits=x, validate_args=False).log_prob(idx.long()).unsqueeze(-1)
        assert bool(torch.isclose(lp, want, rtol=1e-5, atol=1e-5).all()), float((lp - want).abs().max())
        times = {k: [] for k in paths}
        for fn in paths.values():
            for _ in range(3):
                fn()
        for _ in range(o.rounds):
            for k, fn in paths.items():                                # alternating rounds
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(o.iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / o.iters)
        nbytes = B * K * 4 + B * (1 + 4 + 4 + 4)                        # logits and dones in; int32 action, float32 action, log-prob out
        for k in paths:
            t = sorted(times[k])
            rec = dict(rows=B, n_actions=K, path=k, us_median=round(t[len(t) // 2], 1), us_min=round(t[0], 1), us_max=round(t[-1], 1),
                       fused_bytes=nbytes, rounds=o.rounds, iters=o.iters)
            rows_out.append(rec)
            print(json.dumps(rec), flush=True)
    print("%9s %3s %6s %12s %22s" % ("rows", "K", "path", "us (median)", "range"))
    for rec in rows_out:
        print("%9d %3d %6s %12.1f %10.1f .. %-9.1f" % (rec["rows"], rec["n_actions"], rec["path"], rec["us_median"], rec["us_min"], rec["us_max"]))
    print("per act, enqueue included (the loop does not wait for the device between acts); not measured: the gain in a real step next to the policy's forward")


if __name__ == "__main__":
    main()
