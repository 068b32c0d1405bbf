"""What the edge list of one 8192-row PPO minibatch costs on one MI355X, from the compact adjacency and from the entity table, at the c3, c4 and c5-shard
shapes (T = 25, feed-forward, max_edge_dist 1.0 — the reference's default):

  new_exact   gmpe.minibatch.Gather.edges, exact mode: count call, one read of the count, write call (gmpe_minibatch_edges)
  new_cap     the same with cap = the count rounded up to 64 Ki: one call, no host synchronisation
  parent      what the library could do before: gmpe_minibatch_gather materialising only the adj batch [rows, E, E], then gmpe_edges_from_adj on it (int32 ids
              widened to int64, one read of the count)
  torch_x1/2  the adj batch materialised the same way, then the torch-op restatement of process_adj (gnn_new.py:329-358: mask, multiply, nonzero, index) once
              and twice — what the unchanged policy runs in actor and critic

The inputs are entity tables with positions uniform in the world and no masked node; the compact matrices are gmpe_expand_adj of them, so every path sees the
same graphs and the edge lists are compared (exactly) before anything is timed. Each (shape, form) runs in a fresh child process, under its own time limit, and
the run stops at the first child that fails. In a child the paths alternate for `--rounds` rounds of `--batches` consecutive minibatches; a round is timed with a
host clock around work that ends in a device synchronise. Reported: the median over all rounds of `--procs` processes with the range, bytes read and written per
minibatch computed from the shapes, and the achieved rate against the fill ceilings of profiles/r04_fillbw.json.

    python tools/minibatch_edges_bw.py [--procs 3] [--rounds 5] [--batches 20] > profiles/minibatch_edges_bw.log
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

JULY = "nav_metered_one_goal_graph_rotate_tube_july"
SHAPES = {
    "c3": dict(scenario_name=JULY, num_envs=4096, num_agents=10, num_obstacles=0, num_walls=0, world_size=4.0, episode_length=25),
    "c4": dict(scenario_name="navigation_graph", num_envs=8192, num_agents=32, num_obstacles=8, num_walls=4, world_size=8.0, episode_length=25),
    "c5shard": dict(scenario_name="navigation_graph", num_envs=2048, num_agents=64, num_obstacles=0, num_walls=0, world_size=12.0, episode_length=25),
}
ROWS, D_EDGE = 8192, 1.0
PATHS = ("new_exact", "new_cap", "parent", "torch_x1", "torch_x2")


def process_adj(torch, adj, d):
    """the torch ops of TransformerConvNet.process_adj for a [B, E, E] batch"""
    mask = ((adj < d) & (adj > 0)).float()
    adj = adj * mask
    idx = adj.nonzero(as_tuple=False)
    attr = adj[idx[:, 0], idx[:, 1], idx[:, 2]]
    base = idx[:, 0] * adj.shape[1]
    return torch.stack([base + idx[:, 1], base + idx[:, 2]], dim=0), attr.unsqueeze(1)


def child(shape, form, rounds, batches):
    import torch
    import gmpe
    from gmpe import _lib
    from gmpe.engine import GmpeEngine, expand_adj
    from gmpe.minibatch import Gather
    kw = SHAPES[shape]
    cfg = gmpe.make_config(**kw)
    T, N, A, E, W = cfg.episode_length, cfg.num_envs, cfg.num_agents, cfg.num_entities, cfg.entity_table_width
    g = torch.Generator(device="cuda"); g.manual_seed(0)
    tab = torch.rand((T + 1, N, W), generator=g, device="cuda", dtype=torch.float64) * kw["world_size"]
    tab[..., W - (E + 31) // 32:] = 0                                    # no masked entity
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device="cuda")
    arrays = dict(obs=z(T + 1, N, A, 1), agent_id=z(T + 1, N, A, 1, dt=torch.int32), masks=z(T + 1, N, A, 1), active_masks=z(T + 1, N, A, 1), entity_table=tab)
    if form == "compact":
        arrays["adj"] = expand_adj(cfg, tab)
    # Gather checks obs against cfg.obs_dim only through its shape [T+1, N, A, D]: D = 1 keeps the unused fields small
    gat = Gather(cfg, arrays)
    src_kind, src = gat._edge_source
    lib = _lib.load()
    eng = GmpeEngine(gmpe.make_config(**dict(kw, num_envs=8)))          # the handle gmpe_edges_from_adj wants (its workspace); no env of it is stepped
    perm = torch.randperm(T * N * A, generator=g, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    plan = _lib.GmpeMinibatchPlan()
    plan.mode, plan.num_fields, plan.T, plan.N, plan.A, plan.L = _lib.MB_FEED_FORWARD, 1, T, N, A, 1
    f = plan.fields[0]
    f.kind = _lib.MB_ENV_ROW if form == "compact" else _lib.MB_TABLE_ADJ
    f.row_bytes, f.slot_stride, f.src = E * E * 4, src.stride(0) * src.element_size(), src.data_ptr()
    plan.perm, plan.perm_len, plan.rows = perm.data_ptr(), perm.shape[0], ROWS

    def adj_batch(off):
        out = torch.empty((ROWS, E, E), device="cuda")
        plan.offset, f.dst = off, out.data_ptr()
        _lib.check(lib.gmpe_minibatch_gather(C.byref(cfg), 0, C.byref(plan), stream), "gmpe_minibatch_gather")
        return out

    first = gat.edges(perm, 0, ROWS, D_EDGE)
    n = first.n_edges
    cap = -(-n // 65536) * 65536 + 65536
    run = dict(
        new_exact=lambda off: gat.edges(perm, off, ROWS, D_EDGE),
        new_cap=lambda off: gat.edges(perm, off, ROWS, D_EDGE, cap=cap),
        parent=lambda off: eng.edges_from_adj(adj_batch(off), D_EDGE, cap=cap, index64=True),
        torch_x1=lambda off: process_adj(torch, adj_batch(off), D_EDGE),
        torch_x2=lambda off: (lambda a: (process_adj(torch, a, D_EDGE), process_adj(torch, a, D_EDGE)))(adj_batch(off)),
    )
    # the same edges from every path, before anything is timed
    capped, par, tor = run["new_cap"](0), run["parent"](0), run["torch_x1"](0)
    assert int(capped.n_edges.item()) == n == par[2] == tor[0].shape[1]
    for ei, ea in ((capped.edge_index[:, :n], capped.edge_attr[:n]), (par[0], par[1].view(-1, 1)), tor):
        assert torch.equal(ei, first.edge_index) and torch.equal(ea.view(torch.int32), first.edge_attr.view(torch.int32))
    offs = [(i * ROWS) % (perm.shape[0] - ROWS) for i in range(batches)]
    times = {p: [] for p in PATHS}
    for p in PATHS:                                                      # warm-up of every path and shape
        for off in offs[:3]:
            run[p](off)
    for _ in range(rounds):
        for p in PATHS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for off in offs:
                run[p](off)
            torch.cuda.synchronize()
            times[p].append((time.perf_counter() - t0) * 1e6 / batches)
    src_graph = E * E * 4 if form == "compact" else W * 8
    batch_bytes = ROWS * E * E * 4
    rd = dict(new_exact=2 * ROWS * src_graph, new_cap=2 * ROWS * src_graph, parent=ROWS * src_graph + 2 * batch_bytes,
              torch_x1=None, torch_x2=None)
    wr = dict(new_exact=n * 20, new_cap=n * 20, parent=batch_bytes + n * 12 + n * 16, torch_x1=None, torch_x2=None)
    print(json.dumps(dict(shape=shape, form=form, E=E, rows=ROWS, n_edges=n, share=round(n / (ROWS * E * (E - 1)), 4), adj_batch_MB=round(batch_bytes / 1e6, 1),
                          us={p: [round(x, 1) for x in times[p]] for p in PATHS}, read_bytes=rd, written_bytes=wr)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--shapes", default="c3,c4,c5shard")
    ap.add_argument("--child", nargs=2, metavar=("SHAPE", "FORM"))
    ap.add_argument("--limit", type=int, default=150, help="seconds one child process may take")
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.child[1], args.rounds, args.batches)
    fill = json.load(open(os.path.join(ROOT, "profiles", "r04_fillbw.json")))["fill_GBps"]
    results = {}
    for proc in range(args.procs):
        for shape in args.shapes.split(","):
            for form in ("compact", "table"):
                cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", shape, form, "--rounds", str(args.rounds),
                       "--batches", str(args.batches)]
                out = subprocess.run(cmd, capture_output=True, text=True)
                if out.returncode != 0:                                  # nothing more is started on the device after a failure
                    sys.stderr.write(out.stdout + out.stderr)
                    raise SystemExit("child %s %s failed with %d: stopping" % (shape, form, out.returncode))
                row = json.loads(out.stdout.strip().splitlines()[-1])
                print(json.dumps(dict(row, process=proc)), flush=True)
                r = results.setdefault((shape, form), dict(row, us={p: [] for p in PATHS}))
                for p in PATHS:
                    r["us"][p] += row["us"][p]
    print()
    print("median us per minibatch over %d processes x %d rounds x %d minibatches [min - max]; GB/s = (read + written bytes) / median; fill ceilings %s"
          % (args.procs, args.rounds, args.batches, fill))
    print("%-8s %-8s %4s %10s %6s  %-10s %9s %20s %9s %9s %8s %11s" % ("shape", "form", "E", "edges", "share", "path", "median", "range", "read MB", "write MB",
                                                                         "GB/s", "vs parent"))
    for (shape, form), r in results.items():
        base = statistics.median(r["us"]["parent"])
        for p in PATHS:
            med, lo, hi = statistics.median(r["us"][p]), min(r["us"][p]), max(r["us"][p])
            rd, wr = r["read_bytes"][p], r["written_bytes"][p]
            rate = "%8.0f" % ((rd + wr) / med / 1e3) if rd is not None else "       -"
            frac = " (%.2f of the %s ceiling)" % ((rd + wr) / med / 1e3 / fill["98MB" if rd + wr < 200e6 else "2.5GB"], "98MB" if rd + wr < 200e6 else "2.5GB") \
                if rd is not None else ""
            print("%-8s %-8s %4d %10d %6.3f  %-10s %9.1f %20s %9s %9s %s %10.2fx%s" % (
                shape, form, r["E"], r["n_edges"], r["share"], p, med, "[%.1f - %.1f]" % (lo, hi), "-" if rd is None else "%.1f" % (rd / 1e6),
                "-" if wr is None else "%.1f" % (wr / 1e6), rate, med / base, frac))


if __name__ == "__main__":
    main()
