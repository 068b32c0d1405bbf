"""What the GNNBase forward costs at E = 128 on one MI355X (gmpe.gnn_base_wide / gnn_base_wide_from_table), by the method of tools/gnn_base_time.py:

  wide_rows    gmpe.gnn_base_wide on a real engine's node rows and compact adjacency (one matrix per 64 consecutive rows): one launch
  wide_table   gmpe.gnn_base_wide_from_table on the same engine's fp64 entity table (table_share = 64): one launch, neither array read
  torch        the restatement of tests/gnn_lib.py as device torch ops on the same rows, the adjacency materialised first (timed with it): the only
               other way to run this module at E = 128 here. It is NOT PyG.
  narrow       gmpe.gnn_base at E = 64 on an engine of 32 agents whose world has the same entity density: the second yardstick, per edge

The engine is bench.py's c5 world (navigation_graph, 64 agents + 64 landmarks, world 12, E = 128), stepped a few steps with random actions; the module
is the shipped actor for the engine's node width, forward under no_grad. `compare`: 256 envs x 64 agents = 16 384 graphs, where the torch edge-list
form fits; `shard`: the kernel alone at the per-GPU shard, 2048 x 64 = 131 072 graphs. HIP events, alternating rounds of `iters` calls after a warm-up
of every path at the timed shape; median and range over the rounds; the results are compared before anything is timed.

--merge label=path.json (repeatable) copies the records of tools/gnn_base_time.py runs into the output under "narrow_path_runs": the narrow path on
the parent build and on this one, run alternately in one session.

    python tools/gnn_wide_time.py [--rounds 5] [--out profiles/gnn_wide_time.json] [--merge parent_1=a.json --merge this_1=b.json ...]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NAV = "navigation_graph"


def stepped_engine(gmpe, torch, np, envs, agents, world, steps=3):
    from gmpe.engine import GmpeEngine
    cfg = gmpe.make_config(scenario_name=NAV, num_envs=envs, num_agents=agents, world_size=world, episode_length=25, seed=5)
    eng = GmpeEngine(cfg, node_form="both", adj_compact=True)
    eng.reset()
    rng = np.random.RandomState(3)
    for _ in range(steps):
        o = eng.step(torch.as_tensor(rng.randint(0, cfg.n_actions, (envs, agents)).astype(np.int32)))
    eng.check_errors()
    N, A, E, F = o.node_obs.shape
    ids = torch.arange(A, device=o.node_obs.device).repeat(N)
    return cfg, eng, o.node_obs.reshape(N * A, E, F).clone(), o.adj.clone(), o.entity_table.clone(), ids


def timed(torch, paths, rounds, iters):
    with torch.no_grad():
        for fn in paths.values():                       # one untimed window per path, at the timed shape
            for _ in range(iters):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in paths}
        for _ in range(rounds):
            for k, fn in paths.items():                 # alternating rounds
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / iters)
    return {k: sorted(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gnn_wide_time.json"))
    ap.add_argument("--merge", action="append", default=[])
    o = ap.parse_args()
    import numpy as np
    import torch
    import gmpe
    import gnn_lib as G
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    recs = []

    def record(shape, E, graphs, edges, times, **more):
        for k, t in times.items():
            med = t[len(t) // 2]
            rec = dict(shape=shape, path=k, graphs=graphs, E=E, edges=edges, us_median=round(med, 1), us_min=round(t[0], 1), us_max=round(t[-1], 1),
                       ns_per_edge_of_median=round(med * 1e3 / edges, 3), us_per_graph_of_median=round(med / graphs, 4), rounds=o.rounds, **more)
            recs.append(rec)
            print(json.dumps(rec), flush=True)

    def module(F):
        return G.build(G.CONFIGS[G.ACTOR if F == 7 else G.ROTATE]).to("cuda").requires_grad_(False)

    # ---- compare: 256 x 64 graphs of E = 128, the wide forward from both sources against the torch restatement
    cfg, eng, x, adj, tab, ids = stepped_engine(gmpe, torch, np, 256, 64, 12.0)
    A, E = cfg.num_agents, cfg.num_entities
    assert E == 128
    base = module(x.shape[-1])
    edges = int(((adj > 0) & (adj < G.MAX_EDGE_DIST)).sum()) * A
    paths = {"wide_rows": lambda: gmpe.gnn_base_wide(x, adj, ids, base),
             "wide_table": lambda: gmpe.gnn_base_wide_from_table(tab, None, ids, base, cfg, table_share=A),
             "torch": lambda: G.forward(base, x, adj.repeat_interleave(A, 0), ids)}
    with torch.no_grad():
        a, t, b = (paths[k]().clone() for k in ("wide_rows", "wide_table", "torch"))
    assert torch.equal(a, t), "the table source does not give the rows' bits"
    # two float32 paths: a pre-activation within rounding of zero may fall on either side of a ReLU's kink (tools/gnn_base_time.py's rule)
    e_row = (a - b).abs().amax(dim=1) / max(1.0, float(b.abs().max()))
    flipped = int((e_row >= 1e-4).sum())
    assert flipped <= a.shape[0] // 1000, flipped
    worst = float(e_row[e_row < 1e-4].max())
    del a, t, b
    record("compare", E, x.shape[0], edges, timed(torch, paths, o.rounds, 5), iters=5, max_rel_diff_vs_torch=worst, rows_across_a_relu_kink=flipped,
           wide_geometry=list(gmpe.gnn.wide_geometry(x.shape[0], E, x.shape[-1])),
           note="torch = the gnn_lib restatement as device torch ops, adjacency materialised and nonzero included; not PyG")
    del paths, x, adj, tab, ids, eng
    torch.cuda.empty_cache()

    # ---- narrow: gnn_base at E = 64, 512 x 32 graphs, a world of the same entity density (12 / sqrt 2)
    cfg, eng, x, adj, tab, ids = stepped_engine(gmpe, torch, np, 512, 32, 8.485)
    A, E = cfg.num_agents, cfg.num_entities
    assert E == 64
    base = module(x.shape[-1])
    edges = int(((adj > 0) & (adj < G.MAX_EDGE_DIST)).sum()) * A
    paths = {"narrow_rows": lambda: gmpe.gnn_base(x, adj, ids, base)}
    record("narrow_same_density", E, x.shape[0], edges, timed(torch, paths, o.rounds, 5), iters=5)
    del paths, x, adj, tab, ids, eng
    torch.cuda.empty_cache()

    # ---- shard: the kernel alone at the per-GPU shard of c5, 2048 x 64 graphs
    cfg, eng, x, adj, tab, ids = stepped_engine(gmpe, torch, np, 2048, 64, 12.0)
    A, E = cfg.num_agents, cfg.num_entities
    base = module(x.shape[-1])
    edges = int(((adj > 0) & (adj < G.MAX_EDGE_DIST)).sum()) * A
    paths = {"wide_rows": lambda: gmpe.gnn_base_wide(x, adj, ids, base),
             "wide_table": lambda: gmpe.gnn_base_wide_from_table(tab, None, ids, base, cfg, table_share=A)}
    with torch.no_grad():
        assert torch.equal(paths["wide_rows"](), paths["wide_table"]())
    record("shard", E, x.shape[0], edges, timed(torch, paths, o.rounds, 3), iters=3)

    out = dict(records=recs, narrow_path_runs={})
    for m in o.merge:
        label, _, path = m.partition("=")
        with open(path) as f:
            out["narrow_path_runs"][label] = json.load(f)
    os.makedirs(os.path.dirname(o.out), exist_ok=True)
    with open(o.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
