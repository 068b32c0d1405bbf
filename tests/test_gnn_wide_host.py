"""Host side of the GNNBase forward on graphs of up to 128 nodes (include/gmpe.h gmpe_gnn_forward_wide / gmpe_gnn_forward_wide_table /
gmpe_gnn_wide_geometry, gmpe.gnn_base_wide, gmpe.gnn_base_wide_from_table), no GPU: the symbols and the constant; every plan refusal of the narrow
entries' tests replayed against the wide ones, with num_nodes 0 and 129 refused and 65 and 128 passing up to the first device call; the Python
refusals by name, the forward-only error where it is raised and where it reaches gmpe.policy.minibatch_losses; the launch geometry against the
restatement of tests/gnn_lib.py; and the compiler's resource reports: the wide kernels without scratch, the narrow ones at their register counts."""
import ctypes as C
import types

import pytest
import torch

import abi_lib
import gmpe
import gnn_lib as G
from gmpe import _lib, gnn as W
from test_gnn_host import MB, TOP, TOP_GRADS, _plan, _refused, _shape
from test_gnn_table_host import config, refused, table_plan, without_cfg

LARGEST = dict(F=16, heads=4, gnn_n=2, embed_n=2, nemb=16, esz=8)               # the largest configuration gnn_base accepts
SHIPPED = dict(F=7, heads=3, gnn_n=2, embed_n=1, nemb=4, esz=2)
NPAIR = 2                                                                       # wave pairs of a workgroup: the most graphs side by side


def nav(agents, **over):
    """navigation_graph with F = 7 node features, the shipped checkpoints' width: E = 2 * agents + obstacles"""
    return gmpe.make_config(scenario_name="navigation_graph", num_envs=2, num_agents=agents, world_size=12.0, graph_feat_type="global", **over)


def restated(rows, E, F, heads, gnn_n, embed_n, nemb, esz):
    """(W, launch LDS, workgroups) of the wide launch from gnn_lib's restated geometry: as many graphs' forward state as fits next to the parameters,
    two at the most; one workgroup per CU's worth of LDS"""
    per, fixed = 4 * G.wave_floats(E, gnn_n + 1, False), 4 * G.n_params(F, heads, gnn_n, embed_n, nemb, esz)
    Wg = min(NPAIR, (G.LDS_CU - fixed) // per)
    assert Wg >= 1
    lds = fixed + Wg * per
    return Wg, lds, min((rows + Wg - 1) // Wg, G.MAX_CU * max(1, min(4, G.LDS_CU // lds)))


def test_symbols_are_exported_and_the_constant_is_mirrored():
    lib = _lib.load()
    assert {"gmpe_gnn_forward_wide", "gmpe_gnn_forward_wide_table", "gmpe_gnn_wide_geometry"} <= set(_lib.SYMBOLS) & abi_lib.exported()
    for f in ("gmpe_gnn_forward_wide", "gmpe_gnn_forward_wide_table", "gmpe_gnn_wide_geometry"):
        assert getattr(lib, f).argtypes is not None
    assert lib.gmpe_abi_version() == 3 and gmpe.config.ABI_VERSION == 3          # added entry points: the ABI version stays
    assert abi_lib.constant("GMPE_GNN_WIDE_MAX_NODES") == _lib.GNN_WIDE_MAX_NODES == W.WIDE_MAX_NODES == 128
    assert abi_lib.constant("GMPE_GNN_MAX_NODES") == _lib.GNN_MAX_NODES == W.MAX_NODES == 64           # the narrow limit stays
    assert gmpe.gnn_base_wide is W.gnn_base_wide and gmpe.gnn_base_wide_from_table is W.gnn_base_wide_from_table


def test_the_wide_entry_refuses_bad_plans_before_any_device_call():
    """test_gnn_host's list for gmpe_gnn_forward, with num_nodes 129 in place of 65"""
    fn = "gmpe_gnn_forward_wide"
    lib = _lib.load()
    assert lib.gmpe_gnn_forward_wide(0, None, None) == -1 and "null plan" in lib.gmpe_last_error().decode()
    for bad, name in ((dict(rows=0), "rows"), (dict(rows=1 << 41), "rows"), (dict(num_nodes=129), "num_nodes"), (dict(num_nodes=0), "num_nodes"),
                      (dict(node_feats=1), "node_feats"), (dict(node_feats=17), "node_feats"), (dict(hidden=64), "hidden"), (dict(heads=5), "heads"),
                      (dict(heads=0), "heads"), (dict(concat=1), "concat"), (dict(beta=1), "beta"), (dict(edge_dim=0), "edge_dim"), (dict(gnn_layer_n=3), "gnn_layer_n"),
                      (dict(embed_layer_n=3), "embed_layer_n"), (dict(embed_layer_n=-1), "embed_layer_n"), (dict(embed_activation=2), "embed_activation"),
                      (dict(conv_activation=-1), "conv_activation"), (dict(embed_layer_norm=2), "embed_layer_norm"), (dict(aggregate=4), "aggregate"),
                      (dict(num_embeddings=17), "num_embeddings"), (dict(embedding_size=0), "embedding_size"), (dict(embedding_size=9), "embedding_size"),
                      (dict(adj_share=0), "adj_share"), (dict(adj_share=4), "adj_share"), (dict(max_edge_dist=float("nan")), "max_edge_dist"),
                      (dict(ln_eps=0.0), "ln_eps"), (dict(node_obs=MB + 2), "node_obs"), (dict(conv1__key_bias=MB + 1), "conv[1].key_bias"),
                      (dict(embed_weight__0=MB + 3), "embed_weight[0]")):
        for E in (20, 65, 128):                         # the narrow shape the list was written for, and both ends of the wide range
            over = dict(num_nodes=E)
            over.update(bad)
            _refused(fn, _plan(**over), name)
    needed = list(TOP) + ["embed_weight__0", "embed_bias__0"] + ["conv%d__%s" % (c, k) for c in range(3) for k in _lib.GNN_CONV_PARAMS] + ["features"]
    for E in (20, 65, 128):                             # 65 and 128 pass the shape's checks: the complaint is the first required pointer
        for k in needed:
            owner, _, name = k.rpartition("__")
            label = "conv[%s].%s" % (owner[4:], name) if owner.startswith("conv") else "%s[%s]" % (owner, name) if owner else k
            _refused(fn, _plan(num_nodes=E, **{k: None}), label, "required")
        nulls = {"conv2__" + k: None for k, _ in _lib.GmpeGnnConv._fields_}
        nulls.update(gnn_layer_n=1, embed_layer_norm=0, ln_weight=None, ln_bias=None, ln_eps=0.0, aggregate=1, agent_id=None, features=None, num_nodes=E)
        _refused(fn, _plan(**nulls), "features")
    assert "1 .. 128" in _message(fn, _plan(num_nodes=129))


def _message(fn, plan):
    lib = _lib.load()
    assert getattr(lib, fn)(0, C.byref(plan), None) == -1
    return lib.gmpe_last_error().decode()


def test_forward_only_plans_pass_every_host_check_at_65_and_128_nodes():
    """no gradient pointer, no workspace: the plans fail at the first device call (there is no device here), not at an argument"""
    lib = _lib.load()
    grads = list(TOP_GRADS) + ["grad_embed_weight__0", "grad_embed_bias__0", "grad_features", "workspace"] + \
        ["conv%d__grad_%s" % (c, k) for c in range(3) for k in _lib.GNN_CONV_PARAMS]
    if torch.cuda.is_available():
        return                                          # fake addresses must not reach a real device
    for E in (1, 64, 65, 128):
        p = _plan(num_nodes=E, workspace_bytes=0, **{k: None for k in grads})
        assert lib.gmpe_gnn_forward_wide(0, C.byref(p), None) == -2, lib.gmpe_last_error().decode()       # GMPE_ERR_HIP: every host check passed
    big = nav(64)
    assert big.num_entities == 128
    for cfg, E in ((config(), 20), (big, 128)):
        tp = table_plan(cfg=cfg, base__num_nodes=E, base__node_feats=cfg.node_feats, table_index=None, table_share=cfg.num_agents,
                        base__rows=2 * cfg.num_agents)
        assert lib.gmpe_gnn_forward_wide_table(0, C.byref(tp), None) == -2, lib.gmpe_last_error().decode()


def test_the_wide_table_entry_refuses_bad_plans_before_any_device_call():
    """test_gnn_table_host's list for gmpe_gnn_forward_table, at its E = 20 and at E = 66 (33 agents)"""
    fn = "gmpe_gnn_forward_wide_table"
    refused(fn, None, "null plan")
    refused(fn, without_cfg(), "cfg", "required")
    wide = nav(33)
    assert wide.num_entities == 66
    for cfg, E in ((None, 20), (wide, 66)):
        plan = lambda **over: table_plan(**dict(dict(cfg=cfg, base__num_nodes=E, base__node_feats=7 if cfg is None else cfg.node_feats), **over))
        refused(fn, plan(table=None), "table", "required")
        refused(fn, plan(base__num_nodes=E - 1), "num_nodes")
        refused(fn, plan(base__node_feats=9), "node_feats")
        refused(fn, plan(table=500 * MB + 4), "table", "8-byte aligned")
        refused(fn, plan(table_index=501 * MB + 4), "table_index", "8-byte aligned")
        refused(fn, plan(table_index=501 * MB + 2, index64=0), "table_index", "4-byte aligned")
        refused(fn, plan(index64=2), "index64")
        refused(fn, plan(table_rows=0), "table_rows")
        refused(fn, plan(table_index=None, table_share=0), "table_share")
        refused(fn, plan(table_index=None, table_share=4), "rows", "multiple of table_share")            # 70 rows
        refused(fn, plan(base__agent_id=None), "agent_id", "required")
        refused(fn, plan(base__agent_id=None, base__aggregate=1), "agent_id", "required")
        refused(fn, plan(base__rows=0), "rows")
        refused(fn, plan(base__heads=5), "heads")
        refused(fn, plan(base__lin1_weight=None), "lin1_weight", "required")
        refused(fn, plan(base__aggregate=4), "aggregate")
        refused(fn, plan(base__features=None), "features")
    refused(fn, table_plan(cfg=config(graph_feat_type="relative")), "node_feats")
    refused(fn, table_plan(cfg=config(num_agents=9)), "num_nodes")
    bad = config()
    bad.abi_version = 99
    refused(fn, table_plan(cfg=bad), "abi_version")
    # more than 128 entities: 64 agents + 64 landmarks + 1 obstacle
    over = nav(64, num_obstacles=1)
    assert over.num_entities == 129
    refused(fn, table_plan(cfg=over, base__num_nodes=129, base__node_feats=over.node_feats), "num_nodes", "1 .. 128")


def test_python_layer_refuses_by_name_before_any_launch():
    z = torch.zeros
    base = G.build(G.CONFIGS[G.ACTOR])
    ids = z(2, dtype=torch.int64)
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="E = 129 nodes: gnn_base_wide is built for at most 128"):
            gmpe.gnn_base_wide(z(2, 129, 7), z(2, 129, 129), ids, base)
        for E in (6, 64, 65, 128):                      # everything in order: the arrays are not on a device
            with pytest.raises(ValueError, match="no CPU fallback"):
                gmpe.gnn_base_wide(z(2, E, 7), z(1, E, E), ids, base)
        with pytest.raises(NotImplementedError, match="adj is .*gnn_base_wide is float32 only"):
            gmpe.gnn_base_wide(z(2, 65, 7), z(2, 65, 65).half(), ids, base)
        with pytest.raises(NotImplementedError, match="gnn_num_heads = 5"):
            gmpe.gnn_base_wide(z(2, 65, 7), z(2, 65, 65), ids, G.build(G.config("random", heads=5)))
        with pytest.raises(ValueError, match="adj must have shape"):
            gmpe.gnn_base_wide(z(2, 65, 7), z(2, 65, 64), ids, base)
        over = nav(64, num_obstacles=1)
        with pytest.raises(NotImplementedError, match="E = 129 nodes: gnn_base_wide is built for at most 128"):
            gmpe.gnn_base_wide_from_table(z(2, over.entity_table_width, dtype=torch.float64), None, z(128, dtype=torch.int64), base, over, table_share=64)
        big = nav(64)
        tab = z(2, big.entity_table_width, dtype=torch.float64)
        with pytest.raises(ValueError, match="no CPU fallback"):
            gmpe.gnn_base_wide_from_table(tab, None, z(128, dtype=torch.int64), base, big, table_share=64)
        with pytest.raises(ValueError, match="entity_table must be float64"):
            gmpe.gnn_base_wide_from_table(tab.float(), None, z(128, dtype=torch.int64), base, big, table_share=64)
    # the narrow forms keep their refusals
    with pytest.raises(NotImplementedError, match="E = 65 nodes: gnn_base is built for at most 64"):
        gmpe.gnn_base(z(2, 65, 7), z(2, 65, 65), ids, base)
    with pytest.raises(NotImplementedError, match="E = 128 nodes: gnn_base is built for at most 64"):
        gmpe.gnn_base_from_table(tab, None, z(128, dtype=torch.int64), base, big, table_share=64)


def test_the_forward_only_error_by_name():
    z = torch.zeros
    base = G.build(G.CONFIGS[G.ACTOR])
    ids = z(2, dtype=torch.int64)
    big = nav(64)
    tab = z(2, big.entity_table_width, dtype=torch.float64)
    assert torch.is_grad_enabled() and all(p.requires_grad for p in base.parameters())
    for E in (6, 65):                                   # whatever E: the wide form has no autograd node
        with pytest.raises(NotImplementedError, match="gnn_base_wide is forward only: backward at E > 64 is not built"):
            gmpe.gnn_base_wide(z(2, E, 7), z(2, E, E), ids, base)
    with pytest.raises(NotImplementedError, match="gnn_base_wide is forward only: backward at E > 64 is not built"):
        gmpe.gnn_base_wide_from_table(tab, None, z(128, dtype=torch.int64), base, big, table_share=64)
    # under no_grad, and with frozen parameters, the call goes on to the next check: the arrays are not on a device
    with torch.no_grad():
        with pytest.raises(ValueError, match="no CPU fallback"):
            gmpe.gnn_base_wide(z(2, 65, 7), z(2, 65, 65), ids, base)
    for p in base.parameters():
        p.requires_grad_(False)
    with pytest.raises(ValueError, match="no CPU fallback"):
        gmpe.gnn_base_wide(z(2, 65, 7), z(2, 65, 65), ids, base)
    with pytest.raises(ValueError, match="no CPU fallback"):
        gmpe.gnn_base_wide_from_table(tab, None, z(128, dtype=torch.int64), base, big, table_share=64)


def test_training_at_65_nodes_raises_the_forward_only_error_through_minibatch_losses():
    from gmpe import policy as P
    z = torch.zeros
    net = types.SimpleNamespace(gnn_base=G.build(G.CONFIGS[G.ACTOR]))
    rows = 4
    sample = [z(rows, 6), z(rows, 6), z(rows, 65, 7), z(rows, 65, 65), z(rows, 1, dtype=torch.int64), z(rows, 1, dtype=torch.int64), z(rows, 1, 64),
              z(rows, 1, 64)] + [z(rows, 1)] * 8
    with pytest.raises(NotImplementedError, match="gnn_base_wide is forward only: backward at E > 64 is not built"):
        P.minibatch_losses(net, net, tuple(sample), types.SimpleNamespace())
    # the table form of the same minibatch
    big = nav(33)
    rows_t = gmpe.minibatch.TableRows(z(2, big.entity_table_width, dtype=torch.float64), z(rows, dtype=torch.int64), big)
    sample[2], sample[3] = None, rows_t
    with pytest.raises(NotImplementedError, match="gnn_base_wide is forward only: backward at E > 64 is not built"):
        P.minibatch_losses(net, net, tuple(sample), types.SimpleNamespace())


def test_the_launch_geometry_is_the_restated_one_and_fits_the_lds():
    for E in (65, 84, 85, 87, 88, 96, 128):
        for conf in (SHIPPED, LARGEST):
            for rows in (1, 2, 513, 5005):
                got = W.wide_geometry(rows, E, conf["F"], conf["heads"], conf["gnn_n"], conf["embed_n"], conf["nemb"], conf["esz"])
                want = restated(rows, E, **conf)
                print("E %3d F %2d rows %4d: W %d, LDS %6d B, %3d workgroups" % ((E, conf["F"], rows) + got))
                assert got == want and got[1] <= 163840 and got[0] in (1, 2)
    # the largest configuration at 128 nodes: 115 200 B of state next to 47 616 B of parameters, 1 KiB to spare
    assert W.wide_geometry(1, 128, **_kw(LARGEST))[:2] == (1, 162816) and 4 * G.n_params(**LARGEST) == 47616 and 4 * G.wave_floats(128, 3, False) == 115200
    # the boundary: two graphs side by side up to E = 87 at the shipped sizes (81 at the largest: 2 x 4 x (6564 + 96 x 81) + 47 616 = 162 336 B), one above
    assert [W.wide_geometry(9, E, 7)[0] for E in (65, 87, 88, 128)] == [2, 2, 1, 1]
    assert [W.wide_geometry(9, E, **_kw(LARGEST))[0] for E in (65, 81, 82, 128)] == [2, 2, 1, 1]
    # at E = 65 the launch has at most 256 workgroups: 513 graphs are 257 tiles, one more
    assert W.wide_geometry(513, 65, 7) == (2, restated(513, 65, **SHIPPED)[1], 256) and W.wide_geometry(511, 65, 7)[2] == 256
    # up to 64 nodes the geometry is the narrow forward's
    for E in (1, 20, 44, 64):
        geo = G.geometry(300, E)
        assert W.wide_geometry(300, E, 7) == (geo["W_fwd"], geo["lds_fwd"], geo["blocks_fwd"])
    lib = _lib.load()
    out = (C.c_int64 * 3)()
    for bad, field in ((dict(E=0), "num_nodes"), (dict(E=129), "num_nodes"), (dict(rows=0), "rows"), (dict(heads=5), "heads"), (dict(F=17), "node_feats")):
        assert lib.gmpe_gnn_wide_geometry(C.byref(_shape(**bad)), out) == -1
        msg = lib.gmpe_last_error().decode()
        assert msg.startswith("gmpe_gnn_wide_geometry:") and field in msg, msg
    assert lib.gmpe_gnn_wide_geometry(C.byref(_shape()), None) == -1 and "out" in lib.gmpe_last_error().decode()
    assert lib.gmpe_gnn_wide_geometry(None, out) == -1 and "null plan" in lib.gmpe_last_error().decode()


def _kw(conf):
    return dict(node_feats=conf["F"], heads=conf["heads"], gnn_layer_N=conf["gnn_n"], embed_layer_N=conf["embed_n"], num_embeddings=conf["nemb"],
                embedding_size=conf["esz"])


def test_the_wide_kernels_use_no_scratch_and_the_narrow_ones_keep_their_registers():
    assert {"gnn", "gnntable", "gnnwide"} <= set(abi_lib.ru_objects())
    wide = abi_lib.kernels("gnnwide", "k_gnn_fwd_wide")
    assert len(wide) == 2 and sum("GnnTableArgs" in n for n in wide) == 1, list(wide)
    for n, r in abi_lib.kernels("gnnwide").items():     # with the finish kernel the shared header defines in every unit that includes it
        print(n, r["VGPRs"], r["AGPRs"], r["ScratchSize"])
        assert r["ScratchSize"] == 0, n
    assert not any(k in n for n in abi_lib.kernels("gnnwide") for k in ("k_gnn_bwd", "k_gnn_fwdI"))      # no second copy of a narrow kernel
    # DESIGN.md 3.13's table: the narrow objects are what they were
    want = {"gnn": {"k_gnn_fwd": (175, 0), "k_gnn_bwd_conv": (256, 256), "k_gnn_bwd_embed": (256, 248), "k_gnn_finish": (16, 0)},
            "gnntable": {"k_gnn_fwd": (173, 0), "k_gnn_bwd_conv": (256, 256), "k_gnn_bwd_embed": (256, 246), "k_gnn_finish": (16, 0)}}
    for obj, ks in want.items():
        rep = abi_lib.kernels(obj)
        assert len(rep) == 4
        for k, regs in ks.items():
            (r,) = [v for n, v in rep.items() if k in n]
            assert (r["VGPRs"], r["AGPRs"]) == regs, (obj, k, r)
