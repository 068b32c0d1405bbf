"""What the policy's masked GRU layer costs on one MI355X, two ways:

  fused   gmpe.rnn_layer: one gmpe_gru_forward launch, and for training one gmpe_gru_backward call (three launches) through autograd
  torch   the path it replaces, written here: nn.GRU + nn.LayerNorm on the device driven by the segment loop — the steps at which any row has a zero mask
          are found with .nonzero().cpu() (a host synchronisation), every segment is one nn.GRU call on the state times the segment's first mask, the
          outputs are concatenated and normalised; backward is torch's autograd

Shapes: training, L = 10 steps of Nb = 51 200 chunks, forward + backward of sum(features * gf) + sum(hxs_out * gh) from leaf x, hxs and parameters; the
rollout step, L = 1, Nb = 40 960, forward only under no_grad. D = H = 64. The masks hold a zero at about 1 step in 25 per row, independently, so at the
training shape every step has a zero in some row and the torch path runs L segments of one step.
Timed with HIP events in alternating rounds of `iters` calls (3 at the training shape, 300 for the rollout step: windows of tens of milliseconds) after a
warm-up of both paths at the timed shape (the comparison run and one untimed window each); median and range over the rounds. The fused results are
compared with the torch ones before anything is timed. FLOP = 2 * 3 * H * (D + H) per row and step forward, three times that with backward.

    python tools/gru_layer_time.py [--rounds 7] [--out profiles/gru_layer_time.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D = H = 64
# iters: calls per timed window, so that a window lasts tens of milliseconds at either shape (a rollout step is a fraction of a millisecond)
SHAPES = [dict(name="train", L=10, Nb=51200, backward=True, iters=3), dict(name="rollout", L=1, Nb=40960, backward=False, iters=300)]


def torch_layer(torch, gru, norm, x, hxs, masks):
    """the segment loop over nn.GRU, then nn.LayerNorm"""
    Nb = hxs.size(0)
    if x.size(0) == Nb:
        out, h = gru(x.unsqueeze(0), (hxs * masks.unsqueeze(-1)).transpose(0, 1).contiguous())
        return norm(out.squeeze(0)), h.transpose(0, 1)
    L = x.size(0) // Nb
    x, masks = x.view(L, Nb, -1), masks.view(L, Nb)
    cuts = (masks[1:] == 0.0).any(dim=-1).nonzero().flatten().cpu().tolist()         # the host synchronisation
    cuts = [0] + [c + 1 for c in cuts] + [L]
    h, outs = hxs.transpose(0, 1), []
    for a, b in zip(cuts[:-1], cuts[1:]):
        o, h = gru(x[a:b], (h * masks[a].view(1, -1, 1)).contiguous())
        outs.append(o)
    return norm(torch.cat(outs, dim=0).reshape(L * Nb, -1)), h.transpose(0, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gru_layer_time.json"))
    o = ap.parse_args()
    import types
    import torch
    import gmpe
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    dev = "cuda"
    recs = []
    for s in SHAPES:
        L, Nb, bwd, iters = s["L"], s["Nb"], s["backward"], s["iters"]
        g = torch.Generator(device=dev)
        g.manual_seed(L * 1000003 + Nb)
        gru, norm = torch.nn.GRU(D, H).to(dev), torch.nn.LayerNorm(H).to(dev)
        with torch.no_grad():
            for p in gru.parameters():
                p.copy_(torch.rand(p.shape, generator=g, device=dev) / 4 - 0.125)
        layer = types.SimpleNamespace(rnn=gru, norm=norm, _recurrent_N=1)
        params = list(gru.parameters()) + list(norm.parameters())
        x = torch.randn((L * Nb, D), generator=g, device=dev).requires_grad_(bwd)
        hxs = (torch.rand((Nb, 1, H), generator=g, device=dev) * 2 - 1).requires_grad_(bwd)
        masks = (torch.rand((L * Nb, 1), generator=g, device=dev) >= 0.04).float()
        gf, gh = torch.randn((L * Nb, H), generator=g, device=dev), torch.randn((Nb, 1, H), generator=g, device=dev)
        ws = torch.empty((gmpe.rnn_workspace_bytes(L, Nb, H, backward=bwd),), dtype=torch.uint8, device=dev)
        paths = {"fused": lambda: gmpe.rnn_layer(x, hxs, masks, layer, workspace=ws if bwd else None),
                 "torch": lambda: torch_layer(torch, gru, norm, x, hxs, masks)}

        def run(fn):
            if not bwd:
                with torch.no_grad():
                    f, h = fn()
                return [f, h]
            f, h = fn()
            return [f.detach(), h.detach()] + list(torch.autograd.grad((f * gf).sum() + (h * gh).sum(), [x, hxs] + params))
        chk = {k: [t.clone() for t in run(fn)] for k, fn in paths.items()}
        worst = 0.0
        for a, b in zip(chk["fused"], chk["torch"]):
            e = float((a - b).abs().max() / max(1.0, float(b.abs().max())))
            worst = max(worst, e)
            assert e < 1e-4, e                          # two float32 paths; the weight gradients are float32 sums over 512 000 rows on the torch side
        del chk
        times = {k: [] for k in paths}
        for fn in paths.values():                       # one untimed window per path
            for _ in range(iters):
                run(fn)
        torch.cuda.synchronize()
        for _ in range(o.rounds):
            for k, fn in paths.items():                 # alternating rounds
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    run(fn)
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / iters)
        flop = 2 * 3 * H * (D + H) * L * Nb * (3 if bwd else 1)
        for k in paths:
            t = sorted(times[k])
            rec = dict(shape=s["name"], L=L, Nb=Nb, D=D, H=H, backward=bwd, path=k, us_median=round(t[len(t) // 2], 1), us_min=round(t[0], 1),
                       us_max=round(t[-1], 1), GFLOP=round(flop / 1e9, 2), TFLOPs=round(flop / t[len(t) // 2] / 1e6, 2), max_rel_diff_vs_torch=worst,
                       rounds=o.rounds, iters=iters, zero_mask_rate=0.04)
            recs.append(rec)
            print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(o.out), exist_ok=True)
    with open(o.out, "w") as f:
        json.dump(recs, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
