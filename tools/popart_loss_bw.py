"""What the loss arithmetic of one PPO minibatch WITH PopArt costs on one MI355X, forward + backward, two ways:

  fused   gmpe.ppo_losses_popart: one gmpe_ppo_loss_popart call (four launches) forward — value head, PopArt.update, the losses, the three gradients of
          the head, the rescaled layer; backward multiplies the stored gradients by the incoming scalars
  torch   the chain it replaces, as device torch ops with their autograd backward: F.linear(features, W, b); PopArt.update + normalize restated on
          device tensors (new weight / bias / stddev tensors, as the reference's new Parameters); the thirty-odd loss ops of ppo_update; float32

Both start from leaf logits [rows, K], critic features [rows, H] and the layer's weight / bias, and end with the two .backward() calls of ppo_update.
Shapes: rows = 25 * 4096 * A / num_mini_batch at H = 64, K = 25 — c2 / c3 (A = 10) with num_mini_batch 1, 4 and 32, and A = 3 with 1. Timed with HIP
events in alternating rounds after a warm-up; median and range over the rounds. Bytes = what a fused pass must move once: the features read once and
grad_features written once (2 * rows * H * 4), logits + available_actions + grad_logits (3 * rows * K * 4), twelve [rows] columns (the fused row pass
reads the features a second time for grad_features / grad_weight; that read is of a tile the same workgroup has just read). GB/s against the fill
ceiling of profiles/r04_fillbw.json. The fused results are checked against the torch ones before anything is timed.

    python tools/popart_loss_bw.py [--rounds 7] [--iters 5]      # one JSON line per (shape, path) + a summary table
"""
import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, K = 64, 25
SHAPES = [25 * 4096 * 10 // 32, 25 * 4096 * 10 // 4, 25 * 4096 * 3, 25 * 4096 * 10]
ARGS = types.SimpleNamespace(clip_param=0.2, huber_delta=10.0, entropy_coef=0.01, use_policy_active_masks=True, use_value_active_masks=True,
                             use_clipped_value_loss=True, use_huber_loss=True, use_valuenorm=False, use_popart=True)


class PA(object):
    """The tensors of PopArt(H, 1) on the device after some training: a non-trivial mean and stddev."""

    def __init__(self, torch, w, b):
        dev = "cuda"
        self.weight, self.bias = torch.nn.Parameter(w.clone()), torch.nn.Parameter(b.clone())
        self.stddev, self.mean, self.mean_sq = torch.full((1,), 0.7, device=dev), torch.full((1,), 0.01, device=dev), torch.full((1,), 0.6, device=dev)
        self.debiasing_term = torch.tensor(0.05, device=dev)
        self.beta, self.epsilon, self.norm_axes, self.output_shape = 0.99999, 1e-5, 1, 1


def torch_losses(torch, logits, feats, f, pa, a=ARGS):
    values = torch.nn.functional.linear(feats, pa.weight, pa.bias)
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
    with torch.no_grad():                                              # PopArt.update (popart.py:62-83)
        old_mean, old_stddev = pa.mean, pa.stddev
        pa.mean.mul_(pa.beta).add_(R.mean(dim=0) * (1.0 - pa.beta))
        pa.mean_sq.mul_(pa.beta).add_((R ** 2).mean(dim=0) * (1.0 - pa.beta))
        pa.debiasing_term.mul_(pa.beta).add_(1.0 * (1.0 - pa.beta))
        pa.stddev = (pa.mean_sq - pa.mean ** 2).sqrt().clamp(min=1e-4)
        new_w = pa.weight * old_stddev / pa.stddev
        new_b = (old_stddev * pa.bias + old_mean - pa.mean) / pa.stddev
    mean = pa.mean / pa.debiasing_term.clamp(min=pa.epsilon)
    var = (pa.mean_sq / pa.debiasing_term.clamp(min=pa.epsilon) - mean ** 2).clamp(min=1e-2)
    Rn = (R - mean[None]) / torch.sqrt(var)[None]

    def huber(e, d):
        return (abs(e) <= d).float() * e ** 2 / 2 + (e > d).float() * d * (abs(e) - d / 2)
    L = torch.max(huber(Rn - values, a.huber_delta), huber(Rn - vpc, a.huber_delta))
    return policy - ent * a.entropy_coef, (L * am).sum() / am.sum(), (new_w, new_b)


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
    for B in SHAPES:
        g = torch.Generator(device="cuda")
        g.manual_seed(B)
        r = lambda *s: torch.randn(s, generator=g, device="cuda")
        logits, feats = r(B, K).requires_grad_(True), r(B, H).requires_grad_(True)
        w0, b0 = r(1, H) / 8, r(1) / 8
        act = torch.randint(0, K, (B, 1), generator=g, device="cuda")
        avail = (torch.rand((B, K), generator=g, device="cuda") < 0.8).float()
        avail.scatter_(1, act, 1.0)
        f = dict(actions=act.float(), value_preds=r(B, 1), returns=3 * r(B, 1), active_masks=(torch.rand((B, 1), generator=g, device="cuda") < 0.8).float(),
                 old_action_log_probs=-np.log(K) + 0.2 * r(B, 1), adv_targ=r(B, 1), available_actions=avail)
        ws = torch.empty((gmpe.ppo_loss.popart_workspace_bytes(B, H),), dtype=torch.uint8, device="cuda")

        def fused(pa):
            res = gmpe.ppo_losses_popart(logits, feats, f, ARGS, pa, workspace=ws)
            return res.actor_loss, res.value_loss, (pa.weight, pa.bias)

        def run(fn, pa):
            logits.grad = feats.grad = None
            w, b = pa.weight, pa.bias
            a, v, new = fn(pa)
            a.backward()
            (v * 1.0).backward()
            return a.detach(), v.detach(), logits.grad, feats.grad, w.grad, b.grad, new[0].detach(), new[1].detach()
        paths = {"fused": fused, "torch": lambda pa: torch_losses(torch, logits, feats, f, pa)}
        chk = {k: [t.clone() for t in run(fn, PA(torch, w0, b0))] for k, fn in paths.items()}
        for x, y in zip(chk["fused"], chk["torch"]):
            # scalars agree; a gradient row may differ where a comparison (ratio vs a clip bound, ...) falls within float32 rounding of a tie
            # (grad_weight / grad_bias are float32 sums over all rows on the torch side: they get the looser absolute term)
            bad = ~torch.isclose(x, y, rtol=2e-4, atol=(1e-6 if x.numel() > H else 1e-4) * float(y.abs().max()) + 1e-12)
            assert float(bad.float().mean()) <= (1e-5 if x.numel() > H else 0.0), (float(bad.float().mean()), float((x - y).abs().max()))
        times = {k: [] for k in paths}
        for k, fn in paths.items():
            run(fn, PA(torch, w0, b0))
        for _ in range(o.rounds):
            for k, fn in paths.items():                                # alternating rounds; a fresh layer per round, built outside the timed window
                pas = [PA(torch, w0, b0) for _ in range(o.iters)]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for pa in pas:
                    run(fn, pa)
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / o.iters)
        nbytes = 2 * B * H * 4 + 3 * B * K * 4 + 12 * B * 4
        for k in paths:
            t = sorted(times[k])
            rec = dict(rows=B, hidden=H, n_actions=K, path=k, us_median=round(t[len(t) // 2], 1), us_min=round(t[0], 1), us_max=round(t[-1], 1), bytes=nbytes,
                       GBps=round(nbytes / t[len(t) // 2] / 1e3, 1), fill_ceiling_GBps=ceil, rounds=o.rounds, iters=o.iters)
            rows_out.append(rec)
            print(json.dumps(rec), flush=True)
    print("%9s %4s %3s %6s %12s %22s %9s %8s" % ("rows", "H", "K", "path", "us (median)", "range", "GB/s", "of fill"))
    for rec in rows_out:
        print("%9d %4d %3d %6s %12.1f %10.1f .. %-9.1f %9.1f %7.1f%%" % (rec["rows"], rec["hidden"], rec["n_actions"], rec["path"], rec["us_median"], rec["us_min"],
                                                                       rec["us_max"], rec["GBps"], 100.0 * rec["GBps"] / ceil))


if __name__ == "__main__":
    main()
