"""Edge lists of PPO minibatches on the device (gmpe_minibatch_edges; gmpe.minibatch.Gather.edges / edge_list; DeviceRolloutBuffer adj="edges" / step_edges).
Every comparison is exact: ids and counts as integers, edge_attr as bits. The reference is tests/mb_edges_lib.py, which tests/test_minibatch_edges_host.py pins to
the reference's own process_adj; the synthetic inputs are checked there on the CPU, the engine-driven ones here (on the NumPy side, before the kernel's output
is looked at).

1. golden: the fixture's buffer uploaded, every minibatch of both generators, both thresholds, int64 and int32 ids;
2. the three storage forms of engine rollouts (goal reaches and resets inside) give identical lists, equal to the rule applied to the gather's adj batch;
3. shapes: E and rows sweeps, feed-forward / recurrent (T % L == 0 and != 0), identity permutation, out-of-range entries, cap below / at / above the count with
   a guard region, inclusive, count-only + write == one call, the scalar-load path on a source that is not 16-byte aligned;
4. DeviceRolloutBuffer: adj="edges" against adj="matrix", step_edges across storage forms;
5. determinism of outputs and workspace; 6. capture in a graph."""
import ctypes as C
import os

import numpy as np
import pytest

import gmpe
from gmpe import _lib, minibatch  # noqa: F401  (gmpe._lib, gmpe.minibatch)
import mb_edges_lib as EL
import minibatch_lib as M
from test_gpu_gather import JULY, _queue

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "minibatch_edges.npz")
GOLD_IN = os.path.join(HERE, "golden", "minibatch_generators.npz")
ROT_INV = "nav_graph_metered_single_corridor_rot_inv"


def _same(el, ei, ea, what):
    """EdgeList (exact mode) == NumPy (edge_index, edge_attr [n, 1])"""
    got_i, got_a = el.edge_index.cpu().numpy(), el.edge_attr.cpu().numpy()
    assert el.n_edges == ei.shape[1], (what, el.n_edges, ei.shape[1])
    assert got_i.dtype == ei.dtype and got_i.shape == ei.shape and np.array_equal(got_i, ei), what
    assert got_a.dtype == np.float32 and got_a.shape == ea.shape and np.array_equal(got_a.view(np.uint32), ea.view(np.uint32)), what


def test_golden_minibatches_equal_the_reference_process_adj():
    import torch
    from gmpe.minibatch import Gather
    g, gi = np.load(GOLD), np.load(GOLD_IN)
    T, N, A = int(g["T"]), int(g["N"]), int(g["A"])
    cfg = gmpe.make_config(num_envs=N, num_agents=A, episode_length=T)
    assert cfg.num_entities == int(g["E"])
    dev = torch.device("cuda")
    arrays = {k: torch.as_tensor(gi["in_" + k]).to(dev) for k in ("obs", "node_obs", "agent_id", "masks", "active_masks")}
    arrays["adj"] = torch.as_tensor(g["in_adj"]).to(dev)
    seen = 0
    for case in (str(c) for c in g["cases"]):
        nmb, L, rec = int(g[case + "_num_mini_batch"]), int(g[case + "_data_chunk_length"]), bool(g[case + "_recurrent"])
        gather = Gather(cfg, arrays, L if rec else None)
        perm = torch.as_tensor(g[case + "_perm"]).to(dev)
        sampler = M.rec_sampler(T, N, A, nmb, L) if rec else M.ff_sampler(T, N, A, nmb)
        for b, (off, rows) in enumerate(sampler):
            for k, d in enumerate(g["thresholds"]):
                ei, ea = g["%s_%d_d%d_edge_index" % (case, b, k)], g["%s_%d_d%d_edge_attr" % (case, b, k)]
                el = gather.edges(perm, off, rows, float(d))
                assert el.num_graphs == int(g["%s_%d_graphs" % (case, b)]) and el.num_nodes == 6 and el.n_edges == int(g["%s_%d_d%d_n_edges" % (case, b, k)])
                _same(el, ei, ea, (case, b, k, "int64"))
                _same(gather.edges(perm, off, rows, float(d), index64=False), ei.astype(np.int32), ea, (case, b, k, "int32"))
                seen += 1
    assert seen == 22


def _engine_rollout(torch, kw, T, queue):
    """one rollout kept in the three storage forms: materialised, compact, table only"""
    from gmpe.engine import GmpeEngine
    from gmpe.rollout import DeviceRolloutBuffer
    cfg = gmpe.make_config(**kw)
    N, A = cfg.num_envs, cfg.num_agents
    engines = [GmpeEngine(cfg), GmpeEngine(cfg, adj_compact=True), GmpeEngine(cfg, adj_compact=True, node_form="table", adj_form="none")]
    bufs = [DeviceRolloutBuffer(e, T) for e in engines]
    for b in bufs:
        b.warmup()
    if queue:
        _queue(engines[0], engines, np.random.RandomState(4), N, A)        # goal reaches within the rollout
    g = torch.Generator(device="cuda"); g.manual_seed(7)
    acts = torch.where(torch.rand((T, N, A), generator=g, device="cuda") < 0.7, torch.full((T, N, A), 14, device="cuda"),
                       torch.randint(0, cfg.n_actions, (T, N, A), generator=g, device="cuda")).to(torch.int32)
    for b in bufs:
        b.collect(acts)
    return cfg, bufs, g


ROLLOUTS = {
    "july_4096x10": (dict(scenario_name=JULY, num_envs=4096, num_agents=10, world_size=4.0, episode_length=35, seed=31), 40, True, 1.0),
    "rot_inv_F7": (dict(scenario_name=ROT_INV, num_envs=64, num_agents=4, world_size=2.4, episode_length=35, seed=32), 40, True, 1.0),
    "obstacles_E44": (dict(scenario_name="navigation_graph", num_envs=48, num_agents=32, num_obstacles=8, num_walls=4, world_size=8.0, episode_length=3, seed=33),
                      5, False, 3.0),
}


@pytest.mark.parametrize("name", sorted(ROLLOUTS))
def test_storage_forms_agree_on_engine_rollouts(name):
    import torch
    kw, T, queue, d = ROLLOUTS[name]
    cfg, bufs, g = _engine_rollout(torch, kw, T, queue)
    N, A, E, L = cfg.num_envs, cfg.num_agents, cfg.num_entities, 4
    assert (name != "rot_inv_F7" or cfg.node_feats == 7) and (name != "obstacles_E44" or E >= 44)
    rows_ff, rows_rec = min(8192, T * N * A // 2), min(2048, T * N * A // L // 2)
    perm_ff = torch.randperm(T * N * A, generator=g, device="cuda")
    perm_rec = torch.randperm(T * N * A // L, generator=g, device="cuda")
    assert int(bufs[0].dones.sum()) > 0                                   # episodes ended inside the rollout: resets (and, queued, goal reaches) happened
    for rec, perm, off, rows in ((False, perm_ff, 5, rows_ff), (True, perm_rec, 3, rows_rec)):
        gathers = [gmpe.minibatch.Gather(cfg, b.minibatch_arrays(), L if rec else None) for b in bufs]
        assert [x._edge_source[0] for x in gathers] == [gmpe._lib.MBE_ADJ, gmpe._lib.MBE_ADJ_COMPACT, gmpe._lib.MBE_TABLE]
        batch = gathers[0](perm, off, rows)["adj"].cpu().numpy()           # what gmpe_minibatch_gather materialises
        c = dict(EL.conditions(batch, d), masked_nodes=int(((batch == 0).all(1) & (batch == 0).all(2)).sum()))
        print(name, "recurrent" if rec else "feed-forward", "graphs", batch.shape[0], c)
        assert 0.05 <= c["share"] <= 0.95, c
        assert c["masked"] >= 1, "no masked node in a graph with edges: the mask words would not matter"
        for inclusive in (False, True):
            ei, ea, _ = EL.edges(batch, d, inclusive)
            for form, x in zip(("materialised", "compact", "table"), gathers):
                _same(x.edges(perm, off, rows, d, inclusive=inclusive), ei, ea, (name, rec, form, inclusive))
    for b in bufs:
        b.engine.check_errors()


def _compact(torch, E, rows, L=None):
    adj, perm, off = EL.shape_case(E, rows, L)
    return adj, perm, off, torch.as_tensor(adj).cuda(), torch.as_tensor(perm).cuda()


def _edge_list(src, E, d, perm, off, rows, L=None, source=None, **kw):
    from gmpe.minibatch import edge_list
    T, N, A = EL.SHAPE_TNA
    return edge_list(None, src.device, gmpe._lib.MBE_ADJ_COMPACT if source is None else source, src, T, N, A, E, d, perm=perm, offset=off, rows=rows,
                     data_chunk_length=L, **kw)


@pytest.mark.parametrize("E", EL.SHAPE_E)
def test_shapes_by_E(E):
    import torch
    T, N, A = EL.SHAPE_TNA
    rows = 65
    adj, perm, off, adj_d, perm_d = _compact(torch, E, rows)
    adj5 = np.ascontiguousarray(adj[:, :, None].repeat(A, 2))
    adj5[:, :, 1:] = adj5[:, :, 1:] * np.float32(0.5)                      # the ego copies differ (ties stay ties: halves of multiples of 0.25 against 1.0)
    adj5_d = torch.as_tensor(adj5).cuda()
    shifted = torch.zeros(adj_d.numel() + 1, device="cuda")[1:].view(adj_d.shape)   # 4-byte aligned only: the scalar-load path whatever E is
    shifted.copy_(adj_d)
    assert shifted.data_ptr() % 16 == 4
    for inclusive in (False, True):
        ei, ea, _ = EL.minibatch_edges(adj[:, :, None].repeat(A, 2), perm, off, rows, T, N, A, EL.SYN_D, inclusive=inclusive)
        for what, src in (("aligned", adj_d), ("shifted", shifted)):
            _same(_edge_list(src, E, EL.SYN_D, perm_d, off, rows, inclusive=inclusive), ei, ea, (E, inclusive, what))
        _same(_edge_list(adj_d, E, EL.SYN_D, perm_d, off, rows, inclusive=inclusive, index64=False), ei.astype(np.int32), ea, (E, inclusive, "int32"))
        ei5, ea5, _ = EL.minibatch_edges(adj5, perm, off, rows, T, N, A, EL.SYN_D, inclusive=inclusive)
        _same(_edge_list(adj5_d, E, EL.SYN_D, perm_d, off, rows, source=gmpe._lib.MBE_ADJ, inclusive=inclusive), ei5, ea5, (E, inclusive, "per ego"))
    assert E < 3 or not np.array_equal(ei, ei5)


@pytest.mark.parametrize("L", [None, 5, 4])
@pytest.mark.parametrize("rows", EL.SHAPE_ROWS)
def test_shapes_by_rows(rows, L):
    import torch
    T, N, A = EL.SHAPE_TNA
    E = 20
    adj, perm, off, adj_d, perm_d = _compact(torch, E, rows, L)
    ei, ea, _ = EL.minibatch_edges(adj[:, :, None].repeat(A, 2), perm, off, rows, T, N, A, EL.SYN_D, L)
    _same(_edge_list(adj_d, E, EL.SYN_D, perm_d, off, rows, L), ei, ea, (rows, L))


@pytest.mark.parametrize("L", [None, 4])
def test_identity_permutation_and_out_of_range_entries(L):
    import torch
    T, N, A = EL.SHAPE_TNA
    E, rows = 20, 17
    adj, perm, off, adj_d, _ = _compact(torch, E, rows, L)
    adj5 = adj[:, :, None].repeat(A, 2)
    ei, ea, _ = EL.minibatch_edges(adj5, None, off, rows, T, N, A, EL.SYN_D, L)
    _same(_edge_list(adj_d, E, EL.SYN_D, None, off, rows, L), ei, ea, "identity")
    n_valid = T * N * A if L is None else T * N * A // L
    perm = perm.copy()
    perm[off + 2], perm[off + 3], perm[off + 9], perm[off + rows - 1] = -1, n_valid, 1 << 40, -(1 << 33)
    ei, ea, counts = EL.minibatch_edges(adj5, perm, off, rows, T, N, A, EL.SYN_D, L)
    bad = np.tile(np.isin(np.arange(rows), [2, 3, 9, rows - 1]), 1 if L is None else L)
    assert (counts[bad] == 0).all() and counts[~bad].sum() > 0 and (counts[np.flatnonzero(bad)[:-1] + 1] > 0).any()
    _same(_edge_list(adj_d, E, EL.SYN_D, torch.as_tensor(perm).cuda(), off, rows, L), ei, ea, "out of range")
    # the identity past the end of the samples: graphs without edges
    ei, ea, counts = EL.minibatch_edges(adj5, None, n_valid - 5, 9, T, N, A, EL.SYN_D, L)
    assert (counts.reshape(-1, 9)[:, 5:] == 0).all()
    _same(_edge_list(adj_d, E, EL.SYN_D, None, n_valid - 5, 9, L), ei, ea, "identity past the end")


def _raw(torch, src, E, perm, off, rows, cap, index64, L=None, guard=64, ws=None, count_only=False, reuse=False, inclusive=False):
    """one gmpe_minibatch_edges call on caller-owned outputs with a guard region behind each: -> (edge_index buffer, edge_attr buffer, n_edges, workspace)"""
    from gmpe import _lib
    lib = _lib.load()
    T, N, A = EL.SHAPE_TNA
    graphs = rows * (L or 1)
    nb = C.c_size_t()
    assert lib.gmpe_minibatch_edges_workspace_bytes(graphs, C.byref(nb)) == 0
    ws = torch.zeros(nb.value, dtype=torch.uint8, device="cuda") if ws is None else ws
    ei = torch.full((2 * cap + guard,), -7, dtype=torch.int64 if index64 else torch.int32, device="cuda")
    ea = torch.full((cap + guard,), -7.0, dtype=torch.float32, device="cuda")
    ne = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    p = _lib.GmpeMbEdgesPlan()
    p.mode, p.source, p.T, p.N, p.A, p.L, p.E = (_lib.MB_RECURRENT if L else _lib.MB_FEED_FORWARD), _lib.MBE_ADJ_COMPACT, T, N, A, L or 1, E
    p.inclusive, p.index64, p.reuse_counts, p.max_edge_dist = int(inclusive), int(index64), int(reuse), EL.SYN_D
    p.perm, p.perm_len, p.offset, p.rows = perm.data_ptr(), perm.shape[0], off, rows
    p.src, p.slot_stride = src.data_ptr(), src.stride(0) * 4
    if not count_only:
        p.edge_index, p.edge_attr, p.cap = ei.data_ptr(), ea.data_ptr(), cap
    p.n_edges, p.workspace, p.workspace_bytes = ne.data_ptr(), ws.data_ptr(), nb.value
    _lib.check(lib.gmpe_minibatch_edges(None, 0, C.byref(p), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "gmpe_minibatch_edges")
    torch.cuda.synchronize()
    return ei, ea, ne, ws


@pytest.mark.parametrize("index64", [True, False])
def test_cap_below_at_and_above_the_count_with_a_guard_region(index64):
    import torch
    T, N, A = EL.SHAPE_TNA
    E, rows = 20, 65
    adj, perm, off, adj_d, perm_d = _compact(torch, E, rows)
    ei, ea, _ = EL.minibatch_edges(adj[:, :, None].repeat(A, 2), perm, off, rows, T, N, A, EL.SYN_D, dtype=np.int64 if index64 else np.int32)
    n = ei.shape[1]
    assert n > 1000
    for cap in (1, 63, n // 2, n - 1, n, n + 1, n + 500):
        gi, ga, ne, _ = _raw(torch, adj_d, E, perm_d, off, rows, cap, index64)
        m = min(n, cap)
        gi, ga = gi.cpu().numpy(), ga.cpu().numpy()
        assert int(ne.item()) == n, cap                                          # the true count whatever cap is
        assert np.array_equal(gi[:m], ei[0, :m]) and np.array_equal(gi[cap:cap + m], ei[1, :m]), cap
        assert np.array_equal(ga[:m].view(np.uint32), ea[:m, 0].view(np.uint32)), cap
        assert (gi[m:cap] == -7).all() and (gi[cap + m:] == -7).all() and (ga[m:] == -7.0).all(), cap      # nothing past the edges, nothing past cap


def test_count_only_then_write_equals_one_call():
    import torch
    E, rows, L = 20, 1025, 4
    adj, perm, off, adj_d, perm_d = _compact(torch, E, rows, L)
    _, _, ne, ws = _raw(torch, adj_d, E, perm_d, off, rows, 0, True, L, count_only=True)
    n = int(ne.item())
    assert n > 0
    one = _raw(torch, adj_d, E, perm_d, off, rows, n, True, L)
    two = _raw(torch, adj_d, E, perm_d, off, rows, n, True, L, ws=ws.clone(), reuse=True)
    assert int(one[2].item()) == n and int(two[2].item()) == -7                  # the write-only call leaves n_edges alone
    assert torch.equal(one[0], two[0]) and torch.equal(one[1].view(torch.int32), two[1].view(torch.int32)) and torch.equal(one[3], ws) and torch.equal(two[3], ws)
    assert not (one[0][:2 * n] == -7).any()


def test_two_calls_give_identical_bytes():
    import torch
    E, rows = 44, 1025
    adj, perm, off, adj_d, perm_d = _compact(torch, E, rows)
    a = _raw(torch, adj_d, E, perm_d, off, rows, 500000, True, inclusive=True)
    b = _raw(torch, adj_d, E, perm_d, off, rows, 500000, True, inclusive=True)
    assert 0 < int(a[2].item()) < 500000
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))


def _engine_buffers(torch):
    kw = dict(scenario_name=JULY, num_envs=13, num_agents=4, world_size=2.4, episode_length=6, seed=31)
    return _engine_rollout(torch, kw, 9, True)


def test_buffer_generators_with_edges():
    import torch
    d = 1.0
    cfg, bufs, g = _engine_buffers(torch)
    T, N, A, L = 9, cfg.num_envs, cfg.num_agents, 4
    adv = torch.randn((T, N, A, 1), generator=g, device="cuda")
    perm_ff = torch.randperm(T * N * A, generator=g, device="cuda")
    perm_rec = torch.randperm(T * N * A // L, generator=g, device="cuda")
    for form, b in zip(("materialised", "compact", "table"), bufs):
        for make, perm in ((lambda **kw: b.feed_forward_generator(adv, 3, **kw), perm_ff), (lambda **kw: b.recurrent_generator(adv, 2, L, **kw), perm_rec)):
            matrix = list(make(perm=perm))
            for inclusive in (False, True):
                edges = list(make(perm=perm, adj="edges", max_edge_dist=d, inclusive=inclusive))
                assert len(matrix) == len(edges) > 0
                for tm, te in zip(matrix, edges):
                    assert len(tm) == len(te) == 16
                    for k, (u, v) in enumerate(zip(tm, te)):
                        if k != 3:
                            assert (u is None and v is None) or (u.dtype == v.dtype and torch.equal(u, v)), (form, k)
                    el = te[3]
                    assert isinstance(el, gmpe.minibatch.EdgeList) and el.num_graphs == tm[3].shape[0] and el.num_nodes == tm[3].shape[1]
                    batch = tm[3].cpu().numpy()
                    assert 0.05 <= EL.conditions(batch, d)["share"] <= 0.95
                    ei, ea, _ = EL.edges(batch, d, inclusive)
                    _same(el, ei, ea, (form, inclusive))


def test_step_edges_across_storage_forms():
    import torch
    cfg, bufs, _ = _engine_buffers(torch)
    N, A, E = cfg.num_envs, cfg.num_agents, cfg.num_entities
    for step in (0, 4, 9):
        for inclusive in (False, True):
            for index64 in (True, False):
                want = bufs[1].engine.edges_from_adj_compact(bufs[1]._adj[step], A, 1.0, inclusive=inclusive, index64=index64)
                assert want[2] > 0
                for form, b in zip(("materialised", "compact", "table"), bufs):
                    el = b.step_edges(step, 1.0, inclusive=inclusive, index64=index64)
                    assert (el.num_graphs, el.num_nodes, el.n_edges) == (N * A, E, want[2]), form
                    assert el.edge_index.dtype == want[0].dtype and torch.equal(el.edge_index, want[0]), form
                    assert el.edge_attr.shape == (want[2], 1) and torch.equal(el.edge_attr.view(torch.int32)[:, 0], want[1].view(torch.int32)), form
    capped = bufs[2].step_edges(4, 1.0, cap=10)
    assert capped.edge_index.shape == (2, 10) and capped.n_edges > 10 and torch.equal(capped.edge_index, bufs[1].step_edges(4, 1.0, cap=10).edge_index)


def test_the_call_is_capturable_in_a_graph():
    import torch
    T, N, A = EL.SHAPE_TNA
    E, rows, cap = 20, 1024, 100000
    adj, perm, off, adj_d, perm_d = _compact(torch, E, rows)
    direct = _edge_list(adj_d, E, EL.SYN_D, perm_d, off, rows, cap=cap)
    n = int(direct.n_edges.item())
    assert 0 < n < cap
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                              # one stream, no parallel branches
        captured = _edge_list(adj_d, E, EL.SYN_D, perm_d, off, rows, cap=cap)
    captured.edge_index.fill_(-7); captured.edge_attr.fill_(-7.0); captured.n_edges.fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    assert int(captured.n_edges.item()) == n
    assert torch.equal(captured.edge_index[:, :n], direct.edge_index[:, :n])
    assert torch.equal(captured.edge_attr[:n].view(torch.int32), direct.edge_attr[:n].view(torch.int32))
    assert (captured.edge_index[:, n:] == -7).all() and (captured.edge_attr[n:] == -7.0).all()
    ei, ea, _ = EL.minibatch_edges(adj[:, :, None].repeat(A, 2), perm, off, rows, T, N, A, EL.SYN_D)
    assert np.array_equal(captured.edge_index[:, :n].cpu().numpy(), ei) and np.array_equal(captured.edge_attr[:n].cpu().numpy().view(np.uint32), ea.view(np.uint32))
