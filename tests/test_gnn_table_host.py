"""Host side of the GNNBase from the entity table (include/gmpe.h gmpe_gnn_forward_table / gmpe_gnn_backward_table, gmpe.gnn_base_from_table, adj="table"), no GPU:
the exported symbols and the plan's layout against the header; every refusal of the C entries and of the Python layer by name; the TableRows index arithmetic
against a NumPy restatement of both samplers (csrc/gmpe_mb_map.h), remainders included; adj="table" without a table; graph= and the captured update's
refusal; and the compiler's resource report: no kernel of either GNN object uses scratch memory."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import abi_lib
import gmpe
import gnn_lib as G
from gmpe import _lib, minibatch as MB
from test_gnn_host import MB as MIB, _plan as base_plan

JULY = "nav_metered_one_goal_graph_rotate_tube_july"


def config(**over):
    """E = 20 entities, F = 7 features: the shape test_gnn_host's plans have"""
    kw = dict(scenario_name=JULY, num_envs=4, num_agents=10, graph_feat_type="global")
    kw.update(over)
    return gmpe.make_config(**kw)


def test_symbols_are_exported_and_the_plan_matches_the_header():
    lib = _lib.load()
    assert {"gmpe_gnn_forward_table", "gmpe_gnn_backward_table"} <= set(_lib.SYMBOLS) & abi_lib.exported()
    assert lib.gmpe_abi_version() == 3 and gmpe.config.ABI_VERSION == 3          # added entry points: the ABI version stays
    T = _lib.GmpeGnnTablePlan
    assert abi_lib.layout(T) == abi_lib.mirror_layout(T)
    assert abi_lib.layout(_lib.GmpeGnnPlan) == abi_lib.mirror_layout(_lib.GmpeGnnPlan)                   # the wrapped plan is unchanged
    assert T.base.offset == 0 and T.base.size == C.sizeof(_lib.GmpeGnnPlan) == 8 + 16 * 4 + 2 * 8 + 8 * 8 + 4 * 8 + 5 * 8 + 4 * 8 + 3 * 144 + 4 * 8
    assert C.sizeof(T) == C.sizeof(_lib.GmpeGnnPlan) + 4 * 8 + 2 * 4
    assert [f[0] for f in T._fields_] == ["base", "cfg", "table", "table_rows", "table_index", "index64", "table_share"]
    assert gmpe.gnn_base_from_table is gmpe.gnn.gnn_base_from_table
    cfg = config()
    assert cfg.num_entities == 20 and cfg.node_feats == 7


def table_plan(cfg=None, **over):
    """a table plan over fake, well separated addresses around test_gnn_host's base plan: nothing here reaches a device"""
    tp = _lib.GmpeGnnTablePlan()
    base_over = dict(node_obs=None, adj=None, adj_share=0)                      # none of the three is read
    base_over.update({k[6:]: over.pop(k) for k in list(over) if k.startswith("base__")})
    tp.base = base_plan(**base_over)
    tp._cfg = cfg if cfg is not None else config()
    tp.cfg, tp.table, tp.table_rows, tp.table_index, tp.index64, tp.table_share = C.pointer(tp._cfg), 500 * MIB, 12, 501 * MIB, 1, 0
    for k, v in over.items():
        setattr(tp, k, v)
    return tp


def without_cfg():
    tp = table_plan()
    tp.cfg = None
    return tp


def refused(fn, tp, *names):
    lib = _lib.load()
    assert getattr(lib, fn)(0, C.byref(tp) if tp is not None else None, None) == -1
    msg = lib.gmpe_last_error().decode()
    assert msg.startswith(fn + ":") and all(n in msg for n in names), msg


@pytest.mark.parametrize("fn", ["gmpe_gnn_forward_table", "gmpe_gnn_backward_table"])
def test_c_entry_points_refuse_bad_plans_before_any_device_call(fn):
    refused(fn, None, "null plan")
    refused(fn, without_cfg(), "cfg", "required")
    refused(fn, table_plan(table=None), "table", "required")
    refused(fn, table_plan(base__num_nodes=19), "num_nodes")
    refused(fn, table_plan(base__node_feats=8), "node_feats")
    refused(fn, table_plan(cfg=config(graph_feat_type="relative")), "node_feats")          # the cfg's rows have 8 features, the plan 7
    refused(fn, table_plan(cfg=config(num_agents=9)), "num_nodes")
    refused(fn, table_plan(table=500 * MIB + 4), "table", "8-byte aligned")
    refused(fn, table_plan(table_index=501 * MIB + 4), "table_index", "8-byte aligned")
    refused(fn, table_plan(table_index=501 * MIB + 2, index64=0), "table_index", "4-byte aligned")
    refused(fn, table_plan(index64=2), "index64")
    refused(fn, table_plan(table_rows=0), "table_rows")
    refused(fn, table_plan(table_index=None, table_share=0), "table_share")
    refused(fn, table_plan(table_index=None, table_share=4), "rows", "multiple of table_share")          # 70 rows
    refused(fn, table_plan(base__agent_id=None), "agent_id", "required")
    refused(fn, table_plan(base__agent_id=None, base__aggregate=1), "agent_id", "required")              # the view needs its ego with a pool too
    bad = config()
    bad.abi_version = 99
    refused(fn, table_plan(cfg=bad), "abi_version")
    # ... and everything the wrapped plan's own checks refuse, by this function's name
    refused(fn, table_plan(base__rows=0), "rows")
    refused(fn, table_plan(base__heads=5), "heads")
    refused(fn, table_plan(base__lin1_weight=None), "lin1_weight", "required")
    refused(fn, table_plan(base__aggregate=4), "aggregate")
    if fn.startswith("gmpe_gnn_backward"):
        refused(fn, table_plan(base__workspace=None), "workspace")
        refused(fn, table_plan(base__workspace_bytes=64), "workspace_bytes")
        refused(fn, table_plan(base__grad_features=None), "grad_features")
    else:
        refused(fn, table_plan(base__features=None), "features")
    # node_obs, adj and adj_share of the base are not read: the plans above hold none, and these pass every host check
    for tp in (table_plan(), table_plan(index64=0), table_plan(table_index=None, table_share=10), table_plan(base__node_obs=3, base__adj=5, base__adj_share=-7)):
        if not torch.cuda.is_available():               # fake addresses must not reach a real device
            assert getattr(_lib.load(), fn)(0, C.byref(tp), None) == -2, _lib.load().gmpe_last_error().decode()      # GMPE_ERR_HIP: every host check passed


def test_python_layer_refuses_by_name_before_any_launch():
    cfg = config(num_agents=3)                          # E = 6, F = 7, W = cfg.entity_table_width
    W = cfg.entity_table_width
    base = G.build(G.CONFIGS[G.ACTOR])
    tab, idx, ego = torch.zeros(5, 4, W, dtype=torch.float64), torch.zeros(10, dtype=torch.int64), torch.zeros(10, dtype=torch.int64)
    f = gmpe.gnn_base_from_table
    with pytest.raises(ValueError, match="entity_table must be float64"):
        f(tab.float(), idx, ego, base, cfg)
    with pytest.raises(ValueError, match="entity_table and agent_id must be tensors"):
        f(None, idx, ego, base, cfg)
    with pytest.raises(ValueError, match=r"W = cfg.entity_table_width = %d" % W):
        f(torch.zeros(5, 4, W + 1, dtype=torch.float64), idx, ego, base, cfg)
    with pytest.raises(ValueError, match="entity_table must have shape"):
        f(torch.zeros(W, dtype=torch.float64), idx, ego, base, cfg)
    with pytest.raises(ValueError, match="entity_table must be contiguous"):
        f(torch.zeros(5, 4, 2 * W, dtype=torch.float64)[..., ::2], idx, ego, base, cfg)
    with pytest.raises(ValueError, match="table_index must be an int32 or int64 tensor"):
        f(tab, idx.float(), ego, base, cfg)
    with pytest.raises(ValueError, match=r"table_index must have shape \(rows,\)"):
        f(tab, idx.view(5, 2), ego, base, cfg)
    with pytest.raises(ValueError, match="give one of them"):
        f(tab, idx, ego, base, cfg, table_share=3)
    with pytest.raises(ValueError, match="table_share must be an integer >= 1"):
        f(tab, None, ego, base, cfg)
    with pytest.raises(ValueError, match="table_share must be an integer >= 1"):
        f(tab, None, ego, base, cfg, table_share=0)
    with pytest.raises(ValueError, match="agent_id must have shape"):
        f(tab, idx, ego[:9], base, cfg)
    with pytest.raises(ValueError, match=r"agent_id must have shape \(rows,\) or \(rows, 1\) = \(60,\)"):
        f(tab, None, ego, base, cfg, table_share=3)      # 20 table rows x 3
    with pytest.raises(ValueError, match="agent_id must be int32, int64 or float32"):
        f(tab, idx, ego.to(torch.int16), base, cfg)
    with pytest.raises(NotImplementedError, match="3 ids per row"):
        f(tab, idx, torch.zeros(10, 3, dtype=torch.int64), base, cfg)
    # gnn_base's parameter reader and its refusals
    with pytest.raises(ValueError, match="base must have .gnn"):
        f(tab, idx, ego, types.SimpleNamespace(), cfg)
    with pytest.raises(NotImplementedError, match="gnn_num_heads = 5"):
        f(tab, idx, ego, G.build(G.config("random", heads=5)), cfg)
    with pytest.raises(NotImplementedError, match=r"entity_embed.weight is .*float32 only"):
        f(tab, idx, ego, G.build(G.config("random")).to(torch.bfloat16), cfg)
    rel = config(num_agents=3, graph_feat_type="relative")                      # F = 8 rows into a module built for F = 7
    with pytest.raises(ValueError, match=r"lin1.weight must have shape \(16, 10\)"):
        f(torch.zeros(5, 4, rel.entity_table_width, dtype=torch.float64), idx, ego, base, rel)
    # the issue's "32-agent + 8-obstacle + 4-wall" config has 72 entities: more nodes than the kernels are built for
    big = gmpe.make_config(scenario_name="navigation_graph", num_envs=2, num_agents=32, num_obstacles=8, num_walls=4, world_size=8.0)
    assert big.num_entities == 72
    with pytest.raises(NotImplementedError, match="E = 72 nodes"):
        f(torch.zeros(2, big.entity_table_width, dtype=torch.float64), None, torch.zeros(64, dtype=torch.int64), G.build(G.config("rotate")), big, table_share=32)
    # everything in order: the arrays are not on a device
    for args, kw in (((tab, idx, ego), {}), ((tab, idx.to(torch.int32), ego.view(10, 1).float()), {}), ((tab[0], None, torch.zeros(12)), dict(table_share=3))):
        with pytest.raises(ValueError, match="no CPU fallback"):
            f(args[0], args[1], args[2], base, cfg, **kw)


def sample_of(perm, off, r, T, N, A, L, chunks):
    """csrc/gmpe_mb_map.h sample_of, restated: output row r -> (t, n, a)"""
    if L is None:
        u = int(perm[off + r])
        t, rem = divmod(u, N * A)
        n, a = divmod(rem, A)
        return t, n, a
    k, l = r % chunks, r // chunks
    f = int(perm[off + k]) * L + l
    n, rem = divmod(f, A * T)
    a, t = divmod(rem, T)
    return t, n, a


@pytest.mark.parametrize("T,N,A,L,nmb", [(5, 3, 2, None, 4), (5, 3, 2, None, 1), (7, 4, 3, None, 5), (5, 3, 2, 4, 2), (7, 4, 3, 10, 3), (6, 2, 3, 3, 4), (9, 1, 1, 2, 2)])
def test_table_rows_index_is_the_samplers_row_map(T, N, A, L, nmb):
    """index[r] = t * N + n of output row r for every minibatch of both samplers: slices of the permutation, remainders never sampled, chunks that cross
    agent and env boundaries when T % L != 0"""
    rng = np.random.RandomState(T * 100 + N * 10 + A)
    if L is None:
        batch, mbs, sampler = MB.feed_forward_sizes(T, N, A, nmb)
        units = batch
        assert sum(r for _, r in sampler) == nmb * mbs <= batch
    else:
        units, mbc, sampler = MB.recurrent_sizes(T, N, A, nmb, L)
        assert sum(r for _, r in sampler) == nmb * mbc <= units and units * L <= T * N * A
    perm = rng.permutation(units)
    seen = 0
    for off, rows in sampler:
        got = MB.table_index(torch.as_tensor(perm)[off:off + rows], T, N, A, L)
        assert got.dtype == torch.int64 and tuple(got.shape) == (rows * (L or 1),)
        want = [t * N + n for t, n, _ in (sample_of(perm, off, r, T, N, A, L, rows) for r in range(rows * (L or 1)))]
        assert got.tolist() == want and (not want or (0 <= min(want) and max(want) < T * N))
        seen += rows
    assert seen > 0
    assert MB.table_index(torch.zeros(0, dtype=torch.int64), T, N, A, L).numel() == 0


def test_adj_table_needs_the_table_and_is_a_known_mode():
    assert MB.ADJ_MODES == ("matrix", "edges", "table") and MB.TableRows._fields == ("table", "index", "cfg")
    MB.check_edge_args("table", None)                   # no max_edge_dist needed: the module's own is used
    cfg = config(num_agents=2)
    z = torch.zeros
    arrays = dict(obs=z(4, 3, 2, cfg.obs_dim), agent_id=z(4, 3, 2, 1, dtype=torch.int32), masks=z(4, 3, 2, 1), active_masks=z(4, 3, 2, 1),
                  node_obs=z(4, 3, 2, 4, 7), adj=z(4, 3, 4, 4))
    with pytest.raises(ValueError, match='adj="table" needs the entity_table'):
        MB.Gather(cfg, arrays, adj="table")
    with pytest.raises(ValueError, match='adj="table" needs the entity_table'):
        next(MB.feed_forward_generator(cfg, arrays, z(3, 3, 2, 1), 1, adj="table"))
    with pytest.raises(ValueError, match='adj="table" needs the entity_table'):
        MB.recurrent_generator(cfg, arrays, z(3, 3, 2, 1), 1, 3, adj="table")
    with pytest.raises(ValueError, match="adj must be one of"):
        MB.Gather(cfg, arrays, adj="rows")


def test_graph_keyword_and_the_captured_updates_refusal():
    from gmpe import policy as P
    for fn in (P.train, P.iteration):
        with pytest.raises(ValueError, match='graph = \'tables\': .* takes "rows"'):
            fn(None, None, None, None, None, types.SimpleNamespace(), graph="tables")
    net = torch.nn.Linear(2, 2)
    opt = torch.optim.Adam(net.parameters())
    rows = MB.TableRows(torch.zeros(2, 3, dtype=torch.float64), torch.zeros(4, dtype=torch.int64), config())
    sample = tuple(rows if i == 3 else (None if i == 2 else torch.zeros(4, 1)) for i in range(16))
    with pytest.raises(NotImplementedError, match="CapturedUpdate: the sample holds a TableRows"):
        P.CapturedUpdate(net, net, opt, opt, sample, types.SimpleNamespace())
    with pytest.raises(NotImplementedError, match="TableRows"):
        P._no_table_rows("CapturedUpdate.update", sample)


def test_no_kernel_of_either_gnn_object_uses_scratch_memory():
    assert {"gnn", "gnntable"} <= set(abi_lib.ru_objects())
    for obj in ("gnn", "gnntable"):
        names, scratch = list(abi_lib.kernels(obj)), abi_lib.scratch(obj, "k_gnn")
        assert len(names) == len(scratch) == 4 and all(s == 0 for s in scratch.values()), (obj, scratch)
        for k in ("k_gnn_fwd", "k_gnn_bwd_conv", "k_gnn_bwd_embed", "k_gnn_finish"):
            assert any(k in n for n in names), (obj, k)
    assert all("GnnTableArgs" in n for n in abi_lib.kernels("gnntable") if "finish" not in n)
    assert not any("GnnTableArgs" in n for n in abi_lib.kernels("gnn"))          # the old object's kernels have no table source
