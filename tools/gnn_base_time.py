"""What the policy's GNNBase costs on one MI355X, two ways:

  fused   gmpe.gnn_base: one gmpe_gnn_forward launch, and for training one gmpe_gnn_backward call (three launches) through autograd
  torch   the restatement of tests/gnn_lib.py run as device torch ops in the same process: process_adj with its nonzero (a host synchronisation), the
          per-edge MLP over the edge list, index_add / scatter_reduce for the aggregation and the softmax; backward is torch's autograd.
          It is NOT PyG: torch_geometric is not installed here, and nothing below says anything about PyG's own kernels.

Shapes, with the shipped actor (F = 7, three heads, two gnn2 layers, one embed layer, ReLU, LayerNorm, graph_aggr = 'node') and gnn_lib's graphs (uniform
positions in a 2.4-wide square, max_edge_dist = 1: about 7 incoming edges per node at E = 20): the rollout step, 40 960 graphs of E = 20, forward only under
no_grad with the compact adjacency (one matrix per 8 consecutive rows; the torch path has to materialise it first, which is timed with it); the training
minibatch, 8192 graphs of E = 20, forward + backward of sum(features * gf) to every parameter.
Timed with HIP events in alternating rounds of `iters` calls after a warm-up of both paths at the timed shape (the comparison run and one untimed window
each); median and range over the rounds. The fused results are compared with the torch ones before anything is timed.
GFLOP = the model's arithmetic once (2 per multiply-add: lin1's node part per node and edge column per edge, the embed layers per edge, query / key /
value / skip per node and conv, logit and value per edge, head and conv), times 3 for forward + backward; recomputation is not counted.

    python tools/gnn_base_time.py [--rounds 5] [--out profiles/gnn_base_time.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

E, SHARE = 20, 8
SHAPES = [dict(name="rollout", rows=40960, backward=False, iters=10), dict(name="train", rows=8192, backward=True, iters=5)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gnn_base_time.json"))
    o = ap.parse_args()
    import numpy as np
    import torch
    import gmpe
    import gnn_lib as G
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    dev = "cuda"
    cfg = G.CONFIGS[G.ACTOR]
    base = G.build(cfg).to(dev)
    params = list(base.parameters())
    recs = []
    for s in SHAPES:
        rows, bwd, iters = s["rows"], s["backward"], s["iters"]
        rng = np.random.RandomState(rows)
        x, adj, ids = G.draw(rng, rows, E, cfg["F"])
        share = 1 if bwd else SHARE
        x, adj, ids = torch.from_numpy(x).to(dev), torch.from_numpy(adj[::share].copy()).to(dev), torch.from_numpy(ids).to(dev)
        gf = torch.from_numpy(rng.randn(rows, G.C).astype(np.float32)).to(dev)
        edges = int(((adj > 0) & (adj < G.MAX_EDGE_DIST)).sum()) * share
        nbytes = gmpe.gnn_workspace_bytes(rows, E, cfg["F"], backward=bwd)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        paths = {"fused": lambda: gmpe.gnn_base(x, adj, ids, base, workspace=ws if bwd else None),
                 "torch": lambda: G.forward(base, x, adj.repeat_interleave(share, 0) if share > 1 else adj, ids)}

        def run(fn):
            if not bwd:
                with torch.no_grad():
                    return [fn()]
            f = fn()
            return [f.detach()] + list(torch.autograd.grad((f * gf).sum(), params))
        chk = {k: [t.clone() for t in run(fn)] for k, fn in paths.items()}
        # Two float32 paths. A pre-activation within rounding of zero may fall on either side of a ReLU's kink in the two, which changes that graph's row
        # by a finite amount: at most 1 row in 1000 may differ by more than 1e-4 of the largest element; the parameter gradients are held to 1e-2.
        a, b = chk["fused"][0], chk["torch"][0]
        e_row = (a - b).abs().amax(dim=1) / max(1.0, float(b.abs().max()))
        flipped = int((e_row >= 1e-4).sum())
        assert flipped <= rows // 1000, flipped
        worst = float(e_row[e_row < 1e-4].max())
        for a, b in zip(chk["fused"][1:], chk["torch"][1:]):
            e = float((a - b).abs().max()) / max(1.0, float(b.abs().max()))
            assert e < 1e-2, e
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
        H, nconv, nel, K1 = cfg["heads"], cfg["gnn_n"] + 1, cfg["embed_n"], cfg["F"] + cfg["esz"]
        nodes = rows * E
        flop = 2 * (nodes * 16 * (K1 - 1) + edges * (16 + nel * 256) + nconv * (nodes * 256 * (3 * H + 1) + edges * H * 32)) * (3 if bwd else 1)
        for k in paths:
            t = sorted(times[k])
            rec = dict(shape=s["name"], graphs=rows, E=E, edges=edges, adj_share=share, backward=bwd, path=k, us_median=round(t[len(t) // 2], 1),
                       us_min=round(t[0], 1), us_max=round(t[-1], 1), GFLOP=round(flop / 1e9, 3), TFLOPs_of_median=round(flop / t[len(t) // 2] / 1e6, 3),
                       workspace_bytes=nbytes, max_rel_diff_vs_torch=worst, rows_across_a_relu_kink=flipped, rounds=o.rounds, iters=iters,
                       note="torch = the gnn_lib restatement as device torch ops, nonzero included; not PyG")
            recs.append(rec)
            print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(o.out), exist_ok=True)
    with open(o.out, "w") as f:
        json.dump(recs, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
