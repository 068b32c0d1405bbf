"""What the policy's MLPBase costs on one MI355X, two ways:

  fused   gmpe.mlp_base: one gmpe_mlp_forward launch, and for training one gmpe_mlp_backward call (three launches) through autograd
  torch   the path it replaces, on the same device in the same process: torch.cat of the parts, then nn.LayerNorm(D), and per layer nn.Linear, nn.ReLU,
          nn.LayerNorm(64); backward is torch's autograd

Shapes, with the shipped defaults (parts (13, 16), layer_N = 1, ReLU, feature normalisation): the rollout step, 40 960 rows, forward only under no_grad;
the training minibatch, 512 000 rows, forward + backward of sum(features * gf) from leaf parts and parameters.
Timed with HIP events in alternating rounds of `iters` calls (windows of tens of milliseconds) after a warm-up of both paths at the timed shape (the
comparison run and one untimed window each); median and range over the rounds. The fused results are compared with the torch ones before anything is timed.
bytes = what a fused layer has to move: the parts read and the features written once (forward), and for training as much again for the gradients.

    python tools/mlp_base_time.py [--rounds 7] [--out profiles/mlp_base_time.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H = 64
DIMS = (13, 16)
SHAPES = [dict(name="rollout", rows=40960, backward=False, iters=200), dict(name="train", rows=512000, backward=True, iters=5)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp_base_time.json"))
    o = ap.parse_args()
    import types
    import torch
    import gmpe
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    dev, D = "cuda", sum(DIMS)
    recs = []
    for s in SHAPES:
        rows, bwd, iters = s["rows"], s["backward"], s["iters"]
        g = torch.Generator(device=dev)
        g.manual_seed(rows)
        fc = lambda K: torch.nn.Sequential(torch.nn.Linear(K, H), torch.nn.ReLU(), torch.nn.LayerNorm(H)).to(dev)
        base = types.SimpleNamespace(_use_feature_normalization=True, feature_norm=torch.nn.LayerNorm(D).to(dev),
                                     mlp=types.SimpleNamespace(fc1=fc(D), fc2=torch.nn.ModuleList([fc(H)]), _layer_N=1))
        mods = [base.feature_norm, base.mlp.fc1, base.mlp.fc2[0]]
        params = [p for m in mods for p in m.parameters()]
        parts = [torch.randn((rows, d), generator=g, device=dev).requires_grad_(bwd) for d in DIMS]
        gf = torch.randn((rows, H), generator=g, device=dev)
        ws = torch.empty((gmpe.mlp_workspace_bytes(rows, D, 1, backward=bwd),), dtype=torch.uint8, device=dev)
        paths = {"fused": lambda: gmpe.mlp_base(tuple(parts), base, workspace=ws if bwd else None),
                 "torch": lambda: base.mlp.fc2[0](base.mlp.fc1(base.feature_norm(torch.cat(parts, dim=1))))}

        def run(fn):
            if not bwd:
                with torch.no_grad():
                    return [fn()]
            f = fn()
            return [f.detach()] + list(torch.autograd.grad((f * gf).sum(), parts + params))
        chk = {k: [t.clone() for t in run(fn)] for k, fn in paths.items()}
        # Two float32 paths. A pre-activation within rounding of zero may fall on either side of ReLU's kink in the two, which changes that row's part
        # gradients by a finite amount: per-row arrays may differ in at most 1 row in 10 000, the rest within 1e-4. Such a row moves the parameter
        # gradients by its own share (2 rows in 512 000 moved one by 1e-3 of its largest element): they are held to 1e-4 when no row differs, to 1e-2
        # otherwise. The per-row arrays come first in both lists.
        worst, flipped = 0.0, 0
        for a, b in zip(chk["fused"], chk["torch"]):
            scale = max(1.0, float(b.abs().max()))
            if a.dim() == 2 and a.shape[0] == rows:
                e_row = (a - b).abs().amax(dim=1) / scale
                bad = e_row >= 1e-4
                flipped = max(flipped, int(bad.sum()))
                assert int(bad.sum()) <= rows // 10000, int(bad.sum())
                e = float(e_row[~bad].max())
            else:
                e = float((a - b).abs().max()) / scale
                assert e < (1e-2 if flipped else 1e-4), (e, flipped)
            worst = max(worst, e)
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
        nbytes = rows * (D + H) * 4 * (2 if bwd else 1)
        for k in paths:
            t = sorted(times[k])
            rec = dict(shape=s["name"], rows=rows, parts=list(DIMS), layer_N=1, H=H, backward=bwd, path=k, us_median=round(t[len(t) // 2], 1),
                       us_min=round(t[0], 1), us_max=round(t[-1], 1), MB_min=round(nbytes / 1e6, 1), GBs_of_min=round(nbytes / t[len(t) // 2] / 1e3, 1),
                       max_rel_diff_vs_torch=worst, rows_across_a_relu_kink=flipped, rounds=o.rounds, iters=iters)
            recs.append(rec)
            print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(o.out), exist_ok=True)
    with open(o.out, "w") as f:
        json.dump(recs, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
