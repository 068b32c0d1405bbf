"""CPU side of the minibatch edge lists (include/gmpe.h gmpe_minibatch_edges; gmpe.minibatch.Gather.edges; DeviceRolloutBuffer adj="edges" / step_edges): the
exported symbols, the plan struct layout, the argument checks of the C entry point and of the Python wrappers before any launch, the NumPy restatement
(tests/mb_edges_lib.py) against the reference's own process_adj on the reference's own minibatches (tests/golden/minibatch_edges.npz), and the checks that the
inputs of the GPU tests can fail a wrong kernel. All comparisons are exact.

Which input supplies which condition: the golden buffer's envs 0, 1 are real distance matrices of a reference rollout (tests/golden/july_A3_s2_guided.npz) and
supply masked rows and columns; they hold no entry equal to a threshold and no graph without edges (checked below), so envs 2, 3 — synthetic, distances multiples of
0.25, a different matrix per ego — supply the ties, the graphs without an edge and the per-ego difference. The shape sweep's inputs are synthetic throughout.
The engine-driven rollouts of the GPU tests exist only on the device: their conditions are asserted in the GPU test itself, on the NumPy side, before the kernel's
output is looked at."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import abi_lib
import gmpe
from gmpe import _lib
import mb_edges_lib as EL
import minibatch_lib as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "minibatch_edges.npz")
NAMES = ("gmpe_minibatch_edges", "gmpe_minibatch_edges_workspace_bytes")


def test_symbols_are_exported_and_bound():
    assert set(NAMES) <= set(_lib.SYMBOLS) & abi_lib.exported()                  # bound, with the header's parameters: tests/test_abi_host.py


def test_abi_version_is_still_3():
    assert _lib.load().gmpe_abi_version() == 3 and gmpe.config.ABI_VERSION == 3
    assert "#define GMPE_ABI_VERSION 3\n" in open(abi_lib.HDR).read()


FIELDS = ("mode", "source", "T", "N", "A", "L", "E", "inclusive", "index64", "reuse_counts", "max_edge_dist", "reserved", "perm", "perm_len", "offset", "rows",
          "src", "slot_stride", "edge_index", "edge_attr", "cap", "n_edges", "workspace", "workspace_bytes")


def test_plan_struct_layout_matches_c_header():
    P = _lib.GmpeMbEdgesPlan
    assert [f for f, _ in P._fields_] == list(FIELDS)
    assert abi_lib.layout(P) == abi_lib.mirror_layout(P)
    assert [abi_lib.constant("GMPE_MBE_" + k) for k in ("ADJ", "ADJ_COMPACT", "TABLE")] == [_lib.MBE_ADJ, _lib.MBE_ADJ_COMPACT, _lib.MBE_TABLE]


def _plan(**kw):
    """a valid count + write plan on fake device addresses: nothing may be touched before the checks pass"""
    p = _lib.GmpeMbEdgesPlan()
    p.mode, p.source, p.T, p.N, p.A, p.L, p.E = _lib.MB_FEED_FORWARD, _lib.MBE_ADJ_COMPACT, 4, 3, 2, 1, 6
    p.inclusive, p.index64, p.reuse_counts, p.max_edge_dist, p.reserved = 0, 1, 0, 1.0, 0
    p.perm, p.perm_len, p.offset, p.rows = 0x10000, 24, 0, 8
    p.src, p.slot_stride = 0x20000, 3 * 36 * 4
    p.edge_index, p.edge_attr, p.cap, p.n_edges = 0x30000, 0x40000, 100, 0x50000
    p.workspace, p.workspace_bytes = 0x60000, 8 * 2 + 4 * 8
    for k, v in kw.items():
        setattr(p, k, v)
    return p


BAD = [
    dict(mode=7), dict(source=3), dict(source=-1), dict(reserved=1), dict(T=0), dict(N=0), dict(A=0), dict(mode=_lib.MB_RECURRENT, L=0),
    dict(T=1 << 16, N=1 << 16, A=1, slot_stride=1 << 40), dict(E=0), dict(E=161), dict(max_edge_dist=float("nan")), dict(rows=0), dict(offset=-1), dict(offset=20),
    dict(perm_len=0), dict(perm=0x10004), dict(perm=None, offset=1 << 31), dict(index64=0, rows=1 << 29, perm_len=1 << 30, workspace_bytes=1 << 40),
    dict(source=_lib.MBE_TABLE), dict(src=None), dict(slot_stride=3 * 36 * 4 - 4), dict(src=0x20002), dict(slot_stride=3 * 36 * 4 + 2),
    dict(source=_lib.MBE_ADJ), dict(n_edges=None), dict(n_edges=0x50002), dict(workspace=None), dict(workspace=0x60004), dict(workspace_bytes=47), dict(cap=-1),
    dict(edge_attr=None), dict(edge_attr=0x40002), dict(edge_index=0x30004), dict(index64=0, edge_index=0x30002), dict(edge_index=None, reuse_counts=1),
    dict(mode=_lib.MB_RECURRENT, L=3, workspace_bytes=8 * 2 + 4 * 8),
]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: ",".join("%s=%s" % kv for kv in b.items()))
def test_c_entry_point_refuses_bad_plans_before_any_device_call(bad):
    lib = _lib.load()
    assert lib.gmpe_minibatch_edges(None, 0, C.byref(_plan(**bad)), None) == -1
    assert lib.gmpe_last_error().decode().startswith("gmpe_minibatch_edges:")


def test_c_entry_point_checks_the_table_source_against_the_config():
    lib = _lib.load()
    cfg = gmpe.make_config(num_envs=3, num_agents=2, episode_length=4)
    E, W = cfg.num_entities, cfg.entity_table_width
    ok = dict(source=_lib.MBE_TABLE, E=E, slot_stride=3 * W * 8)
    assert lib.gmpe_minibatch_edges(None, 0, C.byref(_plan(**ok)), None) == -1                              # no config
    for bad in (dict(E=E + 1), dict(A=3), dict(slot_stride=3 * W * 8 - 8), dict(src=0x20004), dict(slot_stride=3 * W * 8 + 4)):
        assert lib.gmpe_minibatch_edges(C.byref(cfg), 0, C.byref(_plan(**dict(ok, **bad))), None) == -1, bad
        assert lib.gmpe_last_error().decode().startswith("gmpe_minibatch_edges:")
    stale = gmpe.make_config(num_envs=3, num_agents=2, episode_length=4)
    stale.abi_version = 2
    assert lib.gmpe_minibatch_edges(C.byref(stale), 0, C.byref(_plan(**ok)), None) == -1
    assert lib.gmpe_minibatch_edges(None, 0, None, None) == -1


def test_workspace_bytes():
    lib = _lib.load()
    n = C.c_size_t()
    for graphs in (1, 4, 5, 8192, 8193):
        assert lib.gmpe_minibatch_edges_workspace_bytes(graphs, C.byref(n)) == 0
        assert n.value >= 8 * ((graphs + 3) // 4) + 4 * graphs and n.value % 16 == 0
    assert lib.gmpe_minibatch_edges_workspace_bytes(0, C.byref(n)) == -1
    assert lib.gmpe_minibatch_edges_workspace_bytes(1 << 31, C.byref(n)) == -1
    assert lib.gmpe_minibatch_edges_workspace_bytes(8, None) == -1


def test_python_wrappers_refuse_bad_arguments_before_any_launch():
    from gmpe.minibatch import Gather, check_edge_args, feed_forward_generator, recurrent_generator
    from gmpe.rollout import DeviceRolloutBuffer
    cfg = gmpe.make_config(num_envs=3, num_agents=2, episode_length=4)
    T, N, A, E = 4, 3, 2, cfg.num_entities
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt)
    arrays = dict(obs=z(T + 1, N, A, cfg.obs_dim), agent_id=z(T + 1, N, A, 1, dt=torch.int32), masks=z(T + 1, N, A, 1), active_masks=z(T + 1, N, A, 1),
                  node_obs=z(T + 1, N, A, E, cfg.node_feats), adj=z(T + 1, N, E, E))
    adv = z(T, N, A, 1)
    with pytest.raises(ValueError, match="adj must be one of"):
        feed_forward_generator(cfg, arrays, adv, num_mini_batch=2, adj="edge_list")
    with pytest.raises(ValueError, match="adj must be one of"):
        recurrent_generator(cfg, arrays, adv, 2, 2, adj="sparse")
    with pytest.raises(ValueError, match="max_edge_dist"):
        feed_forward_generator(cfg, arrays, adv, num_mini_batch=2, adj="edges")                 # missing max_edge_dist
    with pytest.raises(ValueError, match="max_edge_dist"):
        recurrent_generator(cfg, arrays, adv, 2, 2, adj="edges", max_edge_dist=float("nan"))
    with pytest.raises(ValueError, match="adj must be one of"):
        Gather(cfg, arrays, adj="both")
    for cap in (0, -5, 2.5):
        with pytest.raises(ValueError, match="cap"):
            check_edge_args("edges", 1.0, cap)
    with pytest.raises(ValueError, match="CUDA"):
        feed_forward_generator(cfg, arrays, adv, num_mini_batch=2, adj="edges", max_edge_dist=1.0)   # host tensors: no CPU fallback
    b = DeviceRolloutBuffer.__new__(DeviceRolloutBuffer)                                       # no engine needed for the checks
    b.T, b.engine = 4, type("Eng", (), dict(N=3, A=2, device=torch.device("cpu"), cfg=cfg))()
    b.obs, b.agent_id, b.masks, b.active_masks = arrays["obs"], arrays["agent_id"], arrays["masks"], arrays["active_masks"]
    b.value_preds = b.returns = b.available_actions = b.entity_table = None
    b._node_obs, b._adj, b.use_centralized_V = arrays["node_obs"], None, True
    with pytest.raises(ValueError, match="adj must be one of"):
        b.feed_forward_generator(adv, 2, adj="list")
    with pytest.raises(ValueError, match="max_edge_dist"):
        b.recurrent_generator(adv, 2, 2, adj="edges")
    with pytest.raises(ValueError, match="adjacency"):
        b.feed_forward_generator(adv, 2, adj="edges", max_edge_dist=1.0)                         # the arrays hold no adjacency form at all
    with pytest.raises(ValueError, match="cap"):
        b.step_edges(0, 1.0, cap=0)
    with pytest.raises(ValueError, match="max_edge_dist"):
        b.step_edges(0, None)
    with pytest.raises(ValueError, match="step"):
        b.step_edges(5, 1.0)
    with pytest.raises(ValueError, match="no adjacency form"):
        b.step_edges(0, 1.0)


def _golden_batches(g):
    T, N, A = int(g["T"]), int(g["N"]), int(g["A"])
    for case in (str(c) for c in g["cases"]):
        perm, nmb, L = g[case + "_perm"], int(g[case + "_num_mini_batch"]), int(g[case + "_data_chunk_length"])
        rec = bool(g[case + "_recurrent"])
        sampler = M.rec_sampler(T, N, A, nmb, L) if rec else M.ff_sampler(T, N, A, nmb)
        assert len(sampler) == int(g[case + "_num_batches"])
        for b, (off, rows) in enumerate(sampler):
            yield case, b, perm, off, rows, (L if rec else None)


def test_numpy_restatement_equals_the_reference_bit_for_bit():
    g = np.load(GOLD)
    T, N, A = int(g["T"]), int(g["N"]), int(g["A"])
    adj = g["in_adj"]
    seen = 0
    for case, b, perm, off, rows, L in _golden_batches(g):
        for k, d in enumerate(g["thresholds"]):
            ei, ea, counts = EL.minibatch_edges(adj, perm, off, rows, T, N, A, d, L)
            ref_ei, ref_ea = g["%s_%d_d%d_edge_index" % (case, b, k)], g["%s_%d_d%d_edge_attr" % (case, b, k)]
            assert ei.dtype == ref_ei.dtype == np.int64 and ei.shape == ref_ei.shape and np.array_equal(ei, ref_ei), (case, b, k)
            assert ea.dtype == ref_ea.dtype == np.float32 and ea.shape == ref_ea.shape and np.array_equal(ea.view(np.uint32), ref_ea.view(np.uint32)), (case, b, k)
            assert int(counts.sum()) == int(g["%s_%d_d%d_n_edges" % (case, b, k)]) == ei.shape[1]
            assert len(counts) == int(g["%s_%d_graphs" % (case, b)])
            seen += 1
    assert seen == 22


def _assert_able_to_fail(batch, d, what):
    c = EL.conditions(batch, d)
    assert 0.05 <= c["share"] <= 0.95, (what, c)
    assert c["empty"] >= 1 and c["masked"] >= 1, (what, c)
    assert c["ties"] >= 1 and c["incl_diff"] >= 1, (what, c)


def test_golden_inputs_can_fail():
    g = np.load(GOLD)
    T, N, A = int(g["T"]), int(g["N"]), int(g["A"])
    adj = g["in_adj"]
    real, syn = adj[:, :2].reshape(-1, 6, 6), adj[:, 2:].reshape(-1, 6, 6)
    assert np.array_equal(adj[:, :2, 0], adj[:, :2, 1]) and np.array_equal(adj[:, :2, 0], adj[:, :2, 2])     # real: the ego copies are one matrix
    assert not np.array_equal(adj[:, 2:, 0], adj[:, 2:, 1])                                                    # synthetic: told apart
    for d in g["thresholds"]:
        cr, cs = EL.conditions(real, d), EL.conditions(syn, d)
        assert cr["masked"] >= 1 and cr["ties"] == 0 and cr["empty"] == 0, cr       # the real matrices supply masked nodes only
        assert cs["ties"] >= 1 and cs["empty"] >= 1 and cs["incl_diff"] >= 1, cs     # the synthetic ones the ties and the graphs without an edge
    for case, b, perm, off, rows, L in _golden_batches(g):
        t, n, a, ok = EL.samples(perm, off, rows, T, N, A, L)
        assert ok.all()
        tn = {}
        for ti, ni, ai in zip(t, n, a):
            tn.setdefault((int(ti), int(ni)), set()).add(int(ai))
        assert any(len(v) >= 2 for v in tn.values()), (case, b)                      # one (t, n) under two or more egos
        for d in g["thresholds"]:
            _assert_able_to_fail(EL.adj_batch(adj, perm, off, rows, T, N, A, L), d, (case, b, float(d)))


@pytest.mark.parametrize("E", EL.SHAPE_E)
def test_shape_sweep_inputs_can_fail_by_E(E):
    T, N, A = EL.SHAPE_TNA
    adj, perm, off = EL.shape_case(E, 65)
    batch = EL.adj_batch(adj[:, :, None].repeat(A, 2), perm, off, 65, T, N, A)
    if E == 2:
        # two nodes: a masked node zeroes the whole graph, so "a masked node in a graph that has edges" cannot exist; the other conditions hold
        c = EL.conditions(batch, EL.SYN_D)
        assert 0.05 <= c["share"] <= 0.95 and c["empty"] >= 1 and c["ties"] >= 1 and c["incl_diff"] >= 1, c
    else:
        _assert_able_to_fail(batch, EL.SYN_D, E)


@pytest.mark.parametrize("rows", EL.SHAPE_ROWS)
@pytest.mark.parametrize("L", [None, 5, 4])
def test_shape_sweep_inputs_can_fail_by_rows(rows, L):
    T, N, A = EL.SHAPE_TNA
    assert T % 5 == 0 and T % 4 != 0
    adj, perm, off = EL.shape_case(20, rows, L)
    if rows == 1:
        # one graph (or the L graphs of one chunk) cannot hold every condition at once: they are checked on the whole source it is drawn from
        _assert_able_to_fail(adj.reshape(-1, 20, 20), EL.SYN_D, "source")
        return
    _assert_able_to_fail(EL.adj_batch(adj[:, :, None].repeat(A, 2), perm, off, rows, T, N, A, L), EL.SYN_D, (rows, L))
