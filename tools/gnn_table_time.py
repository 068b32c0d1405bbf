"""What the policy's GNNBase costs straight from the entity table, against the same GNNBase on arrays that exist, on one MI355X:

  table   gmpe.gnn_base_from_table: the graphs addressed through the fp64 entity table (rollout: the step's [N, W] table with table_share = A; training:
          one int64 per row into the stored [S, N, W] tables)
  rows    gmpe.gnn_base on the materialised arrays: the rollout step's own node_obs [N * A, E, F] and compact adjacency [N, E, E] as the engine wrote them
          (nothing to gather), the training minibatch's [rows, E, F] + [rows, E, E] gathered by the same index first (torch indexing, timed with it:
          it is what the minibatch costs in that form)

The tables are a real engine's (July scenario, 4096 envs x 10 agents: E = 20, F = 8, the shipped F = 8 actor), node_form="both", stepped with random
actions. Shapes: the rollout step, 40 960 graphs, forward under no_grad; the training minibatch, 8192 graphs drawn over the recorded slots, forward +
backward of sum(features * gf) to every parameter. The two paths' results are compared with torch.equal before anything is timed. HIP events, alternating
rounds of `iters` calls after one untimed window each; median and range over the rounds. bytes = what each path allocates per call for the graphs
themselves: the index against the gathered rows and matrices (the rollout step's rows form allocates nothing: its arrays are the engine's outputs).
The table form is not expected to be faster: the GNN's arithmetic dominates, and every graph rebuilds its own E x E matrix. Its purpose is bytes.

    python tools/gnn_table_time.py [--rounds 5] [--out profiles/gnn_table_time.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, A, SLOTS = 4096, 10, 4
SHAPES = [dict(name="rollout", rows=N * A, backward=False, iters=10), dict(name="train", rows=8192, backward=True, iters=5)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gnn_table_time.json"))
    ap.add_argument("--gnn-base", action="append", default=[], metavar="BUILD=JSON",
                    help="a tools/gnn_base_time.py result of the named build (parent, branch) to record next to these: gnn_base itself must not get slower")
    o = ap.parse_args()
    import numpy as np
    import torch
    import gmpe
    import gnn_lib as G
    from gmpe.engine import GmpeEngine
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    dev = "cuda"
    cfg = gmpe.make_config(num_envs=N, num_agents=A, world_size=4.0, episode_length=25, seed=5)     # bench.py's 4096 x 10 world
    E, F, W = cfg.num_entities, cfg.node_feats, cfg.entity_table_width
    base = G.build(G.config("rotate")).to(dev)
    params = list(base.parameters())
    eng = GmpeEngine(cfg, node_form="both", adj_compact=True)
    eng.reset()
    rng = np.random.RandomState(0)
    tabs, rows_, adjs = [], [], []
    for t in range(3 * SLOTS):
        out = eng.step(torch.as_tensor(rng.randint(0, cfg.n_actions, (N, A)).astype(np.int32)))
        if t % 3 == 2:
            tabs.append(out.entity_table.clone()); rows_.append(out.node_obs.clone()); adjs.append(out.adj.clone())
    eng.check_errors()
    tabs, node_obs, adj = torch.stack(tabs), torch.stack(rows_), torch.stack(adjs)
    recs = []
    for s in SHAPES:
        rows, bwd, iters = s["rows"], s["backward"], s["iters"]
        g = torch.Generator().manual_seed(rows)
        gf = torch.randn((rows, G.C), generator=g).to(dev)
        nbytes = gmpe.gnn_workspace_bytes(rows, E, F, backward=bwd)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        if bwd:
            idx = torch.randint(0, SLOTS * N, (rows,), generator=g).to(dev)
            ego = torch.randint(0, A, (rows,), generator=g).to(dev)
            flat_x, flat_a = node_obs.reshape(SLOTS * N, A, E, F), adj.reshape(SLOTS * N, E, E)
            paths = {"table": lambda: gmpe.gnn_base_from_table(tabs, idx, ego, base, cfg, workspace=ws),
                     "rows": lambda: gmpe.gnn_base(flat_x[idx, ego], flat_a[idx], ego, base, workspace=ws)}
            alloc = {"table": rows * 8, "rows": rows * (E * F + E * E) * 4}
        else:
            ego = torch.arange(A, device=dev).repeat(N)
            x1, a1, t1 = node_obs[-1].reshape(rows, E, F), adj[-1], tabs[-1]
            paths = {"table": lambda: gmpe.gnn_base_from_table(t1, None, ego, base, cfg, table_share=A),
                     "rows": lambda: gmpe.gnn_base(x1, a1, ego, base)}
            alloc = {"table": 0, "rows": 0}

        def run(fn):
            if not bwd:
                with torch.no_grad():
                    return [fn()]
            f = fn()
            return [f.detach()] + list(torch.autograd.grad((f * gf).sum(), params))
        chk = {k: [t.clone() for t in run(fn)] for k, fn in paths.items()}
        for a, b in zip(chk["table"], chk["rows"]):
            assert torch.equal(a, b)                    # bit for bit, the features and every parameter gradient
        edges = int(((adj[-1] > 0) & (adj[-1] < G.MAX_EDGE_DIST)).sum()) * A if not bwd else None
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
        for k in paths:
            t = sorted(times[k])
            rec = dict(shape=s["name"], graphs=rows, E=E, F=F, table_width=W, backward=bwd, path=k, us_median=round(t[len(t) // 2], 1),
                       us_min=round(t[0], 1), us_max=round(t[-1], 1), graph_bytes_allocated_per_call=alloc[k],
                       stored_bytes_per_env_step=dict(table=W * 8, rows=(A * E * F + E * E) * 4)[k], workspace_bytes=nbytes, equal_bits=True,
                       rounds=o.rounds, iters=iters)
            if edges is not None:
                rec["edges"] = edges
            recs.append(rec)
            print(json.dumps(rec), flush=True)
    for item in o.gnn_base:                            # tools/gnn_base_time.py's fused records of two builds on the same box, side by side
        build, path = item.split("=", 1)
        for r in json.load(open(path)):
            if r["path"] == "fused":
                recs.append(dict(r, path="gnn_base", build=build, note="tools/gnn_base_time.py, fused path, of the named build"))
    os.makedirs(os.path.dirname(o.out), exist_ok=True)
    with open(o.out, "w") as f:
        json.dump(recs, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
