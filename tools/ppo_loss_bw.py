"""What the loss arithmetic of one PPO minibatch costs on one MI355X, forward + backward, two ways:

  fused   gmpe.ppo_losses: one gmpe_ppo_loss call (four launches) forward; backward multiplies the stored gradients by the incoming scalars
  torch   the same arithmetic as device torch ops with their autograd backward (masked Categorical, ratio / clip / surrogates, ValueNorm.update +
          normalize, clipped huber value loss, masked means), float32, as GR_MAPPO.ppo_update runs it

Both start from leaf logits [rows, K] / values [rows, 1] and end with the two .backward() calls of ppo_update, so each includes the write of
d actor_loss / d logits. Shapes: 8192 and 1 024 000 rows x K = 25 (c3: one target-size minibatch, and one whole rollout with num_mini_batch = 1) and
1 024 000 x 5. Timed with HIP events in alternating rounds after a warm-up; median and range over the rounds. Bytes = what a fused pass must move once:
logits + available_actions + grad_logits (3 * rows * K * 4) plus ten [rows] columns; GB/s against the fill ceiling of profiles/r04_fillbw.json.
The fused results are checked against the torch ones before anything is timed.

    python tools/ppo_loss_bw.py [--rounds 7] [--iters 5]      # one JSON line per (shape, path) + a summary table
"""
import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(8192, 25), (1024000, 25), (1024000, 5)]
ARGS = types.SimpleNamespace(clip_param=0.2, huber_delta=10.0, entropy_coef=0.01, use_policy_active_masks=True, use_value_active_masks=True,
                             use_clipped_value_loss=True, use_huber_loss=True, use_valuenorm=True, use_popart=False)


class VN(object):
    def __init__(self, torch):
        self.running_mean, self.running_mean_sq = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
        self.debiasing_term = torch.zeros((), device="cuda")
        self.beta, self.epsilon, self.norm_axes, self.per_element_update = 0.99999, 1e-5, 1, False


def torch_losses(torch, logits, values, f, vn, a=ARGS):
    x = logits.clone()
    x[f["available_actions"] == 0] = torch.finfo(torch.float32).min
    dist = torch.distributions.Categorical(logits=x, validate_args=False)
    logp = dist.log_prob(f["actions"].squeeze(-1)).unsqueeze(-1)
    am = f["active_masks"]
    ent = (dist.entropy() * am.squeeze(-1)).sum() / am.sum()
    ratio = torch.exp(logp - f["old_action_log_probs"])
    s1, s2 = ratio * f["adv_targ"], torch.clamp(ratio, 1.0 - a.clip_param, 1.0 + a.clip_param) * f["adv_targ"]
    policy = (-torch.sum(torch.min(s1, s2), dim=-1, keepdim=True) * am).sum() / am.sum()
    vp, R = f["value_preds"], f["returns"]
    vpc = vp + (values - vp).clamp(-a.clip_param, a.clip_param)
    with torch.no_grad():
        vn.running_mean.mul_(vn.beta).add_(R.mean(dim=0) * (1.0 - vn.beta))
        vn.running_mean_sq.mul_(vn.beta).add_((R ** 2).mean(dim=0) * (1.0 - vn.beta))
        vn.debiasing_term.mul_(vn.beta).add_(1.0 * (1.0 - vn.beta))
    mean = vn.running_mean / vn.debiasing_term.clamp(min=vn.epsilon)
    var = (vn.running_mean_sq / vn.debiasing_term.clamp(min=vn.epsilon) - mean ** 2).clamp(min=1e-2)
    Rn = (R - mean[None]) / torch.sqrt(var)[None]

    def huber(e, d):
        return (abs(e) <= d).float() * e ** 2 / 2 + (e > d).float() * d * (abs(e) - d / 2)
    L = torch.max(huber(Rn - values, a.huber_delta), huber(Rn - vpc, a.huber_delta))
    return policy - ent * a.entropy_coef, (L * am).sum() / am.sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    o = ap.parse_args()
    import numpy as np
    import torch
    import gmpe
    ceil = json.load(open(os.path.join(ROOT, "profiles", "r04_fillbw.json")))["fill_GBps"]["2.5GB"]
    rows_out = []
    for B, K in SHAPES:
        g = torch.Generator(device="cuda")
        g.manual_seed(B + K)
        r = lambda *s: torch.randn(s, generator=g, device="cuda")
        logits, values = r(B, K).requires_grad_(True), r(B, 1).requires_grad_(True)
        act = torch.randint(0, K, (B, 1), generator=g, device="cuda")
        avail = (torch.rand((B, K), generator=g, device="cuda") < 0.8).float()
        avail.scatter_(1, act, 1.0)
        f = dict(actions=act.float(), value_preds=r(B, 1), returns=3 * r(B, 1), active_masks=(torch.rand((B, 1), generator=g, device="cuda") < 0.8).float(),
                 old_action_log_probs=-np.log(K) + 0.2 * r(B, 1), adv_targ=r(B, 1), available_actions=avail)
        ws = torch.empty((gmpe.ppo_loss.workspace_bytes(B),), dtype=torch.uint8, device="cuda")

        def fused(vn):
            res = gmpe.ppo_losses(logits, values, f, ARGS, vn, workspace=ws)
            return res.actor_loss, res.value_loss

        def run(fn, vn):
            logits.grad = values.grad = None
            a, v = fn(vn)
            a.backward()
            (v * 1.0).backward()
            return a.detach(), v.detach(), logits.grad, values.grad
        paths = {"fused": fused, "torch": lambda vn: torch_losses(torch, logits, values, f, vn)}
        chk = {k: [t.clone() for t in run(fn, VN(torch))] for k, fn in paths.items()}
        for x, y in zip(chk["fused"], chk["torch"]):
            # scalars agree; a gradient row may differ where a comparison (ratio vs a clip bound, ...) falls within float32 rounding of a tie
            bad = ~torch.isclose(x, y, rtol=2e-4, atol=1e-6 * float(y.abs().max()) + 1e-12)
            assert float(bad.float().mean()) <= (1e-5 if x.dim() else 0.0), (float(bad.float().mean()), float((x - y).abs().max()))
        times = {k: [] for k in paths}
        vns = {k: VN(torch) for k in paths}
        for k, fn in paths.items():
            run(fn, vns[k])
        for _ in range(o.rounds):
            for k, fn in paths.items():                                # alternating rounds
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(o.iters):
                    run(fn, vns[k])
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / o.iters)
        nbytes = 3 * B * K * 4 + 10 * B * 4
        for k in paths:
            t = sorted(times[k])
            rec = dict(rows=B, n_actions=K, path=k, us_median=round(t[len(t) // 2], 1), us_min=round(t[0], 1), us_max=round(t[-1], 1), bytes=nbytes,
                       GBps=round(nbytes / t[len(t) // 2] / 1e3, 1), fill_ceiling_GBps=ceil, rounds=o.rounds, iters=o.iters)
            rows_out.append(rec)
            print(json.dumps(rec), flush=True)
    print("%9s %3s %6s %12s %22s %9s %8s" % ("rows", "K", "path", "us (median)", "range", "GB/s", "of fill"))
    for rec in rows_out:
        print("%9d %3d %6s %12.1f %10.1f .. %-9.1f %9.1f %7.1f%%" % (rec["rows"], rec["n_actions"], rec["path"], rec["us_median"], rec["us_min"], rec["us_max"],
                                                                  rec["GBps"], 100.0 * rec["GBps"] / ceil))


if __name__ == "__main__":
    main()
