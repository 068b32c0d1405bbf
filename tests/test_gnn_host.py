"""Host side of the policy's GNNBase (include/gmpe.h gmpe_gnn_forward / gmpe_gnn_backward, gmpe.gnn_base), no GPU:
(a) the restatement of tests/gnn_lib.py: its autograd is the derivative of its forward (central differences, float64); its float32 run stays under the
    1e-5 cap for every array of every case; every ReLU graph meets the margin; the fixture holds the shipped checkpoints' names and shapes; and, where
    torch_geometric is installed, the restatement against the reference's own GNNBase (skipped where these tests were written: it has never run there);
(b) the exported symbols, the plan's layout against the C header, the workspace sizes, the restated launch geometry, and the refusals of both layers;
(c) the compiler's resource report of csrc/gmpe_gnn.hip shows no scratch memory."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import abi_lib
import gmpe
import gnn_lib as G
from gmpe import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "contracts-marl-aam-corridors_amd", "csrc")


# ---------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("case", G.CASES, ids=G.case_id)
def test_the_float32_run_of_the_restatement_stays_under_the_cap(case):
    t64, e_ref = G.truth(*case)
    for k, e in e_ref.items():
        print("%s %-44s err_ref %.3g" % (G.case_id(case), k, e))
    for k, e in e_ref.items():
        assert e <= G.CAP, (case, k, e)
    assert np.abs(t64["features"]).max() > 0


@pytest.mark.parametrize("case", G.CASES, ids=G.case_id)
def test_every_relu_graph_meets_the_margin_and_the_inputs_hold_what_they_promise(case):
    n, E, key, special = case
    cfg = G.CONFIGS[key]
    x, adj, ids, gf, redrawn = G.inputs(*case)
    assert x.shape == (n, E, cfg["F"]) and adj.shape == (n, E, E) and ids.shape == (n,) and gf.shape == (n, G.C)
    assert set(np.unique(x[:, :, -1].numpy())) <= {0.0, 1.0, 2.0} and int(ids.min()) >= 0 and int(ids.max()) < E
    if "ReLU" in (cfg["eact"], cfg["cact"]):
        m = G.margins(G.build(cfg, torch.float64), x, adj, ids)
        print("%s redrawn %d of %d, smallest margin %.3g" % (G.case_id(case), redrawn, n, float(m.min())))
        assert float(m.min()) >= G.MARGIN
    # a graph of E = 20 has some 5e3 pre-activations of density ~0.5 around zero: ~3 % are redrawn; one of E = 64 has 6e4: about every third
    assert redrawn <= (max(2, n // 8) if E <= 20 else n)
    if special:
        mask = ((adj > 0) & (adj < G.MAX_EDGE_DIST)).numpy()
        assert not mask[0].any()                                                    # no edge at all
        assert mask[1][:, 1].sum() == 1 and mask[1][2, 1]                           # node 1 has exactly one incoming edge
        assert mask[2].sum() == E * (E - 1)                                         # complete
        assert not mask[3][1].any() and not mask[3][:, 1].any()                     # a done agent's zeroed row and column
        assert adj[4, 0, 1] == G.MAX_EDGE_DIST and not mask[4][0, 1] and mask[4][1, 0]          # exactly max_edge_dist is excluded
        assert mask[5][0, 1] and not np.tril(mask[5], -1).any()                     # asymmetric: edges from the lower index to the higher only


def test_the_cases_are_the_listed_ones():
    have = {(n, E, k) for n, E, k, _ in G.CASES}
    for n, E in G.SHAPES:
        assert (n, E, G.ACTOR) in have
    for n, E in G.SHAPES[:5]:
        assert (n, E, G.CRITIC) in have
    assert (65, 6, G.ACTOR_MAX) in have and (65, 6, G.ACTOR_ADD) in have and any(k == G.ROTATE for _, _, k in have)
    rnd = [G.CONFIGS[k] for _, _, k in have if k.startswith("random")]
    assert {c["heads"] for c in rnd} >= {1, 4} and {c["gnn_n"] for c in rnd} >= {0, 2} and {c["embed_n"] for c in rnd} >= {0, 2}
    assert {c["eact"] for c in rnd} == {c["cact"] for c in rnd} == {"ReLU", "Tanh"} and {c["ln"] for c in rnd} == {0, 1} and {c["F"] for c in rnd} >= {8, 16}
    assert len(set(G.CASES)) == len(G.CASES) and all(n * E <= 300 * 20 for n, E, _, _ in G.CASES)


def test_the_fixture_holds_the_shipped_names_and_shapes():
    g = G.golden()
    for tag, k1 in (("actor", 9), ("critic", 9), ("rotate", 10)):
        pre = tag + ".gnn_base.gnn."
        assert g[pre + "embed_layer.lin1.weight"].shape == (16, k1) and g[pre + "embed_layer.entity_embed.weight"].shape == (4, 2)
        for conv in ("gnn1", "gnn2.0", "gnn2.1"):
            for lin in ("lin_key", "lin_query", "lin_value"):
                assert g[pre + "%s.%s.weight" % (conv, lin)].shape == (48, 16) and g[pre + "%s.%s.bias" % (conv, lin)].shape == (48,)
            assert g[pre + conv + ".lin_edge.weight"].shape == (48, 1) and pre + conv + ".lin_edge.bias" not in g
            assert g[pre + conv + ".lin_skip.weight"].shape == (16, 16)              # the heads are averaged before the skip
        for s in ("weight", "bias"):                                                # one LayerNorm under two names
            assert np.array_equal(g[pre + "embed_layer.layer_norm." + s], g[pre + "embed_layer.layers.2." + s])
        assert sum(k.startswith(tag + ".") for k in g) == 36
    assert all(v.dtype == np.float32 for v in g.values()) and len(g) == 108


def test_the_parameter_reader_reads_the_fixtures_module():
    from gmpe import gnn as W
    for key in (G.ACTOR, G.CRITIC, G.ROTATE):
        base = G.build(G.CONFIGS[key])
        names, ps, meta = W._base_params(base)
        sd = base.state_dict()
        assert len(names) == len(ps) == 5 + 2 + 3 * 9 and len(set(names)) == len(names)
        for n, p in zip(names, ps):
            k = "gnn." + n.replace("gnn.gnn", "gnn").replace("[", ".").replace("]", "")
            k = k if k in sd else k.replace("gnn.gnn.", "gnn.")
            assert k in sd and sd[k].data_ptr() == p.data_ptr(), (n, k)
        assert {id(p) for p in ps} == {id(p) for p in base.parameters()}             # every parameter once, the shared LayerNorm once
        assert meta == (3, 2, 1, _lib.GNN_RELU, _lib.GNN_RELU, 1, 1e-5, _lib.GNN_MEAN if key == G.CRITIC else _lib.GNN_NODE, 1.0)


def test_autograd_of_the_restatement_is_the_derivative_of_its_forward():
    """central differences in float64 on a 2-graph case, a few coordinates of every parameter, for a ReLU / LayerNorm and a Tanh configuration"""
    for cfg in (G.CONFIGS[G.ACTOR], G._RANDOM[5], G._RANDOM[2]):
        key = G.cfg_key(cfg)
        x, adj, ids, gf, _ = G.inputs(2, 6, key)
        base = G.build(cfg, torch.float64)
        g = G.run(base, x, adj, ids, gf)
        loss = lambda: float((G.forward(base, x.double(), adj.double(), ids) * gf.double()).sum())
        rng = np.random.RandomState(0)
        with torch.no_grad():
            for name, p in base.named_parameters():
                flat = p.view(-1)
                for i in rng.randint(0, flat.numel(), 3):
                    old, h = float(flat[i]), 1e-6
                    flat[i] = old + h
                    up = loss()
                    flat[i] = old - h
                    dn = loss()
                    flat[i] = old
                    num, ana = (up - dn) / (2 * h), g["grad_" + name].reshape(-1)[i]
                    assert abs(num - ana) <= 2e-6 * max(1.0, abs(num)), (key, name, i, num, ana)


def test_the_restatement_against_the_references_gnnbase():
    """The check a user with PyG can run: the reference's own GNNBase (torch_geometric's TransformerConv) with the shipped weights against the restatement,
    float64, outputs and every parameter gradient. torch_geometric is not installed where this was written: this test has never run there."""
    pytest.importorskip("torch_geometric")
    import argparse
    import sys
    ref = os.environ.get("GMPE_REFERENCE")
    if not ref or not os.path.isdir(ref):
        pytest.skip("GMPE_REFERENCE does not name a checkout of the reference")
    sys.path.insert(0, ref)
    from onpolicy.algorithms.utils.gnn_new import GNNBase
    for key in (G.ACTOR, G.CRITIC):
        cfg = G.CONFIGS[key]
        args = argparse.Namespace(num_embeddings=cfg["nemb"], embedding_size=cfg["esz"], embed_hidden_size=16, embed_layer_N=cfg["embed_n"],
                                  embed_use_ReLU=True, embed_add_self_loop=False, gnn_hidden_size=16, gnn_num_heads=cfg["heads"], gnn_concat_heads=False,
                                  gnn_layer_N=cfg["gnn_n"], gnn_use_ReLU=True, max_edge_dist=G.MAX_EDGE_DIST, global_aggr_type="mean", use_orthogonal=True,
                                  use_feature_normalization=True)
        mine = G.build(cfg, torch.float64)
        theirs = GNNBase(args, cfg["F"], 1, "node" if cfg["aggr"] == "node" else "global").double()
        theirs.load_state_dict(mine.state_dict())
        x, adj, ids, gf, _ = G.inputs(33, 20, key)
        a = G.run(mine, x, adj, ids, gf)
        theirs.zero_grad()
        out = theirs(x.double(), adj.double(), ids.view(-1, 1))
        (out * gf.double()).sum().backward()
        assert G.err(out.detach().numpy(), a["features"]) <= 1e-12
        for name, p in theirs.named_parameters():
            assert G.err(p.grad.numpy(), a["grad_" + name]) <= 1e-10, name


# ---------------------------------------------------------------------------------------------- (b)
CONSTS = ("HIDDEN", "MAX_NODES", "MAX_HEADS", "MAX_CONVS", "MAX_EMBED_LAYERS", "MAX_FEATS", "MAX_EMBEDDINGS", "MAX_EMBEDDING_SIZE", "RELU", "TANH", "NODE", "MEAN",
          "MAX", "ADD")


def test_symbols_are_exported_and_the_plan_matches_the_header():
    lib = _lib.load()
    assert {"gmpe_gnn_workspace_bytes", "gmpe_gnn_forward", "gmpe_gnn_backward"} <= set(_lib.SYMBOLS) & abi_lib.exported()
    assert lib.gmpe_abi_version() == 3 and gmpe.config.ABI_VERSION == 3          # added entry points: the ABI version stays
    for T in (_lib.GmpeGnnConv, _lib.GmpeGnnPlan):
        assert abi_lib.layout(T) == abi_lib.mirror_layout(T), T
    assert [abi_lib.constant("GMPE_GNN_" + c) for c in CONSTS] == [getattr(_lib, "GNN_" + c) for c in CONSTS]
    assert C.sizeof(_lib.GmpeGnnConv) == 18 * 8 and C.sizeof(_lib.GmpeGnnPlan) == 8 + 16 * 4 + 2 * 8 + 8 * 8 + 4 * 8 + 5 * 8 + 4 * 8 + 3 * 144 + 4 * 8
    assert gmpe.gnn_base is gmpe.gnn.gnn_base and gmpe.gnn_workspace_bytes is gmpe.gnn.gnn_workspace_bytes


def _shape(rows=70, E=20, F=7, heads=3, gnn_n=2, embed_n=1, nemb=4, esz=2, **over):
    from gmpe import gnn as W
    p = W._shape_plan(rows, E, F, 1, heads, gnn_n, embed_n, nemb, esz)
    for k, v in over.items():
        setattr(p, k, v)
    return p


def test_workspace_bytes_and_the_restated_geometry():
    lib = _lib.load()
    n = C.c_size_t(7)
    assert lib.gmpe_gnn_workspace_bytes(C.byref(_shape()), 0, C.byref(n)) == 0 and n.value == 0          # the forward-only plan takes none
    sizes = []
    for rows in (1, 3, 4, 5, 65, 1000, 1024, 1025, 8192, 40960):
        assert lib.gmpe_gnn_workspace_bytes(C.byref(_shape(rows=rows)), 1, C.byref(n)) == 0
        geo = G.geometry(rows, 20)
        assert n.value == geo["workspace"] == gmpe.gnn_workspace_bytes(rows, 20, 7) and n.value % 8 == 0
        assert n.value >= rows * 20 * 16 * 4 and gmpe.gnn_workspace_bytes(rows, 20, 7, backward=False) == 0
        sizes.append(n.value)
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    # the size is a function of the shapes and the configuration: every other field of the plan may hold anything
    for E, F, heads, gnn_n, embed_n, nemb, esz in ((1, 2, 1, 0, 0, 1, 1), (6, 7, 3, 2, 1, 4, 2), (44, 8, 3, 2, 1, 4, 2), (64, 16, 4, 2, 2, 16, 8), (33, 5, 2, 1, 2, 3, 3)):
        for rows in (1, 9, 5005):
            p = _shape(rows, E, F, heads, gnn_n, embed_n, nemb, esz, embed_activation=9, aggregate=-3, max_edge_dist=float("nan"), workspace_bytes=5)
            assert lib.gmpe_gnn_workspace_bytes(C.byref(p), 1, C.byref(n)) == 0
            geo = G.geometry(rows, E, F, heads, gnn_n, embed_n, nemb, esz)
            assert n.value == geo["workspace"], (rows, E)
            assert geo["lds_fwd"] <= G.LDS_CU and geo["lds_bwd"] <= G.LDS_CU and 1 <= geo["W_bwd"] <= geo["W_fwd"] <= 4
    assert G.geometry(1, 64, 16, 4, 2, 2, 16, 8)["W_bwd"] == 1 and G.geometry(1, 20)["W_bwd"] == 4 and G.geometry(1, 44)["W_bwd"] in (2, 3)
    assert 34 * 1024 <= 4 * G.geometry(1, 20)["np"] <= 36 * 1024                    # "about 35 KB at the shipped sizes"
    for bad, field in ((dict(rows=0), "rows"), (dict(rows=-5), "rows"), (dict(E=0), "num_nodes"), (dict(E=65), "num_nodes"), (dict(F=1), "node_feats"),
                       (dict(F=17), "node_feats"), (dict(heads=0), "heads"), (dict(heads=5), "heads"), (dict(gnn_n=3), "gnn_layer_n"),
                       (dict(gnn_n=-1), "gnn_layer_n"), (dict(embed_n=3), "embed_layer_n"), (dict(nemb=0), "num_embeddings"), (dict(nemb=17), "num_embeddings"),
                       (dict(esz=9), "embedding_size"), (dict(hidden=32), "hidden"), (dict(concat=1), "concat"), (dict(beta=1), "beta"),
                       (dict(edge_dim=2), "edge_dim"), (dict(adj_share=0), "adj_share"), (dict(rows=70, adj_share=4), "multiple of adj_share")):
        assert lib.gmpe_gnn_workspace_bytes(C.byref(_shape(**bad)), 1, C.byref(n)) == -1
        msg = lib.gmpe_last_error().decode()
        assert msg.startswith("gmpe_gnn_workspace_bytes:") and field in msg, msg
    assert lib.gmpe_gnn_workspace_bytes(C.byref(_shape()), 1, None) == -1 and "bytes_out" in lib.gmpe_last_error().decode()
    assert lib.gmpe_gnn_workspace_bytes(C.byref(_shape()), 2, C.byref(n)) == -1 and "want_backward" in lib.gmpe_last_error().decode()
    assert lib.gmpe_gnn_workspace_bytes(None, 1, C.byref(n)) == -1 and "null plan" in lib.gmpe_last_error().decode()
    with pytest.raises(NotImplementedError, match="E = 65"):
        gmpe.gnn_workspace_bytes(10, 65, 7)
    with pytest.raises(NotImplementedError, match="gnn_num_heads = 5"):
        gmpe.gnn_workspace_bytes(10, 20, 7, heads=5)


def test_the_restated_constants_are_the_sources():
    text, host = (open(os.path.join(CSRC, f)).read() for f in ("gmpe_gnn_kernels.h", "gmpe_host.h"))
    for name, want in (("BLOCK", "256"), ("NW", "BLOCK / 64"), ("NINS", "32"), ("QDS", "40"), ("LIN", "C * C + C"), ("MAX_CU", "256"), ("LDS_CU", "160 * 1024")):
        m = re.search(r"\b%s\s*=\s*([^,;]+)[,;]" % name, host if name in ("MAX_CU", "LDS_CU") else text)
        assert m and m.group(1).strip() == want, (name, m and m.group(1))
    assert (G.BLOCK, G.NW, G.NINS, G.QDS, G.LIN, G.MAX_CU, G.LDS_CU) == (256, 4, 32, 40, 272, 256, 160 * 1024) and G.C == _lib.GNN_HIDDEN


MB = 1 << 20
TOP = ("node_obs", "adj", "agent_id", "entity_embed", "lin1_weight", "lin1_bias", "ln_weight", "ln_bias")
TOP_GRADS = ("grad_entity_embed", "grad_lin1_weight", "grad_lin1_bias", "grad_ln_weight", "grad_ln_bias")


def _plan(**over):
    """a plan over fake, well separated addresses (1 MiB apart): nothing here reaches a device. over: field=value, `conv1__key_bias`, `embed_weight__0`"""
    p = _shape()
    p.embed_activation, p.conv_activation, p.embed_layer_norm, p.aggregate, p.max_edge_dist, p.ln_eps = 0, 0, 1, 0, 1.0, 1e-5
    addr = iter(range(MB, 400 * MB, MB))
    for k in TOP + TOP_GRADS + ("features", "grad_features", "workspace"):
        setattr(p, k, next(addr))
    for k in ("embed_weight", "embed_bias", "grad_embed_weight", "grad_embed_bias"):
        getattr(p, k)[0] = next(addr)
    for c in range(3):
        for k, _ in _lib.GmpeGnnConv._fields_:
            setattr(p.conv[c], k, next(addr))
    p.workspace_bytes = 64 * MB
    for k, v in over.items():
        owner, _, name = k.rpartition("__")
        if owner.startswith("conv"):
            setattr(p.conv[int(owner[4:])], name, v)
        elif owner:
            getattr(p, owner)[int(name)] = v
        else:
            setattr(p, k, v)
    return p


def _refused(fn, plan, *names):
    lib = _lib.load()
    assert getattr(lib, fn)(0, C.byref(plan), None) == -1
    msg = lib.gmpe_last_error().decode()
    assert msg.startswith(fn + ":") and all(n in msg for n in names), msg


@pytest.mark.parametrize("fn", ["gmpe_gnn_forward", "gmpe_gnn_backward"])
def test_c_entry_points_refuse_bad_plans_before_any_device_call(fn):
    lib = _lib.load()
    bwd = fn == "gmpe_gnn_backward"
    assert getattr(lib, fn)(0, None, None) == -1 and "null plan" in lib.gmpe_last_error().decode()
    for bad, name in ((dict(rows=0), "rows"), (dict(rows=1 << 41), "rows"), (dict(num_nodes=65), "num_nodes"), (dict(num_nodes=0), "num_nodes"),
                      (dict(node_feats=1), "node_feats"), (dict(node_feats=17), "node_feats"), (dict(hidden=64), "hidden"), (dict(heads=5), "heads"),
                      (dict(heads=0), "heads"), (dict(concat=1), "concat"), (dict(beta=1), "beta"), (dict(edge_dim=0), "edge_dim"), (dict(gnn_layer_n=3), "gnn_layer_n"),
                      (dict(embed_layer_n=3), "embed_layer_n"), (dict(embed_layer_n=-1), "embed_layer_n"), (dict(embed_activation=2), "embed_activation"),
                      (dict(conv_activation=-1), "conv_activation"), (dict(embed_layer_norm=2), "embed_layer_norm"), (dict(aggregate=4), "aggregate"),
                      (dict(num_embeddings=17), "num_embeddings"), (dict(embedding_size=0), "embedding_size"), (dict(embedding_size=9), "embedding_size"),
                      (dict(adj_share=0), "adj_share"), (dict(adj_share=4), "adj_share"), (dict(max_edge_dist=float("nan")), "max_edge_dist"),
                      (dict(ln_eps=0.0), "ln_eps"), (dict(workspace_bytes=64), "workspace_bytes"), (dict(workspace=5 * MB + 4), "workspace"),
                      (dict(node_obs=MB + 2), "node_obs"), (dict(conv1__key_bias=MB + 1), "conv[1].key_bias"), (dict(embed_weight__0=MB + 3), "embed_weight[0]")):
        _refused(fn, _plan(**bad), name)
    needed = list(TOP) + ["embed_weight__0", "embed_bias__0"] + ["conv%d__%s" % (c, k) for c in range(3) for k in _lib.GNN_CONV_PARAMS]
    needed += list(TOP_GRADS) + ["grad_embed_weight__0", "grad_embed_bias__0", "grad_features", "workspace"] + \
        ["conv%d__grad_%s" % (c, k) for c in range(3) for k in _lib.GNN_CONV_PARAMS] if bwd else ["features"]
    for k in needed:
        owner, _, name = k.rpartition("__")
        label = "conv[%s].%s" % (owner[4:], name) if owner.startswith("conv") else "%s[%s]" % (owner, name) if owner else k
        _refused(fn, _plan(**{k: None}), label, "required")
    # what a configuration does not read may be null: conv[2] with gnn_layer_n = 1, the LayerNorm without embed_layer_norm, agent_id with a pool
    nulls = {"conv2__" + k: None for k, _ in _lib.GmpeGnnConv._fields_}
    nulls.update(gnn_layer_n=1, embed_layer_norm=0, ln_weight=None, ln_bias=None, grad_ln_weight=None, grad_ln_bias=None, ln_eps=0.0, aggregate=1, agent_id=None,
                 features=None, grad_features=None)
    _refused(fn, _plan(**nulls), "grad_features" if bwd else "features")            # ... so the first complaint is about the last thing checked


def test_what_each_entry_point_does_not_need_may_be_null():
    """a forward-only plan: no gradient pointers, no workspace; a backward plan: no features. The plans pass the host's checks and fail at the first device
    call (there is no device here): the error is not an argument error."""
    lib = _lib.load()
    grads = list(TOP_GRADS) + ["grad_embed_weight__0", "grad_embed_bias__0", "grad_features"] + \
        ["conv%d__grad_%s" % (c, k) for c in range(3) for k in _lib.GNN_CONV_PARAMS]
    for fn, nulls in (("gmpe_gnn_forward", grads + ["workspace"]), ("gmpe_gnn_backward", ["features"])):
        p = _plan(**{k: None for k in nulls})
        if "workspace" in nulls:
            p.workspace_bytes = 0
        if torch.cuda.is_available():
            continue                                    # fake addresses must not reach a real device
        assert getattr(lib, fn)(0, C.byref(p), None) == -2, lib.gmpe_last_error().decode()          # GMPE_ERR_HIP: every host check passed


def test_python_layer_refuses_what_it_does_not_support():
    z = torch.zeros
    cfg = G.CONFIGS[G.ACTOR]
    x, adj, ids = z(10, 6, 7), z(10, 6, 6), z(10, dtype=torch.int64)
    ok = lambda **over: G.build(G.config("random", **over))
    # NotImplementedError: what is not built
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(NotImplementedError, match="adj is .*float32 only"):
            gmpe.gnn_base(x, adj.to(dt), ids, ok())
        with pytest.raises(NotImplementedError, match=r"entity_embed.weight is .*float32 only"):
            gmpe.gnn_base(x, adj, ids, ok().to(dt))
    with pytest.raises(NotImplementedError, match="E = 65 nodes"):
        gmpe.gnn_base(z(2, 65, 7), z(2, 65, 65), z(2, dtype=torch.int64), ok())
    with pytest.raises(NotImplementedError, match="F = 17"):
        gmpe.gnn_base(z(10, 6, 17), adj, ids, ok(F=17))
    with pytest.raises(NotImplementedError, match="3 ids per row"):
        gmpe.gnn_base(x, adj, z(10, 3, dtype=torch.int64), ok())
    with pytest.raises(NotImplementedError, match="gnn_num_heads = 5"):
        gmpe.gnn_base(x, adj, ids, ok(heads=5))
    with pytest.raises(NotImplementedError, match="gnn_layer_N = 3"):
        gmpe.gnn_base(x, adj, ids, ok(gnn_n=3))
    with pytest.raises(NotImplementedError, match="embed_layer_N = 3"):
        gmpe.gnn_base(x, adj, ids, ok(embed_n=3))
    with pytest.raises(NotImplementedError, match="num_embeddings = 17"):
        gmpe.gnn_base(x, adj, ids, ok(nemb=17))
    with pytest.raises(NotImplementedError, match="embedding_size = 9"):
        gmpe.gnn_base(x, adj, ids, ok(esz=9))
    bad = ok()
    bad.gnn.gnn2[0].concat = True
    with pytest.raises(NotImplementedError, match=r"gnn2\[0\]\.concat is set"):
        gmpe.gnn_base(x, adj, ids, bad)
    bad = ok()
    bad.gnn.gnn1.beta = True
    with pytest.raises(NotImplementedError, match=r"gnn1\.beta is set"):
        gmpe.gnn_base(x, adj, ids, bad)
    bad = ok()
    bad.gnn.edge_dim = 2
    with pytest.raises(NotImplementedError, match="edge_dim = 2"):
        gmpe.gnn_base(x, adj, ids, bad)
    bad = ok()
    bad.gnn.activation = torch.nn.GELU()
    with pytest.raises(NotImplementedError, match="GELU"):
        gmpe.gnn_base(x, adj, ids, bad)
    bad = ok()
    bad.gnn.gnn1.lin_skip = torch.nn.Linear(16, 32)
    with pytest.raises(NotImplementedError, match="gnn_hidden_size = 32"):
        gmpe.gnn_base(x, adj, ids, bad)
    bad = ok()
    bad.gnn.gnn2[1].heads = 2
    with pytest.raises(NotImplementedError, match="one number of heads"):
        gmpe.gnn_base(x, adj, ids, bad)
    # ValueError: what is malformed
    with pytest.raises(ValueError, match="adj must be a tensor"):
        gmpe.gnn_base(x, None, ids, ok())
    with pytest.raises(ValueError, match="node_obs must be float32"):
        gmpe.gnn_base(x.double(), adj, ids, ok())
    with pytest.raises(ValueError, match="agent_id must be int32, int64 or float32"):
        gmpe.gnn_base(x, adj, ids.to(torch.int16), ok())
    with pytest.raises(ValueError, match=r"node_obs must have shape \(rows, E, F\)"):
        gmpe.gnn_base(z(10, 42), adj, ids, ok())
    with pytest.raises(ValueError, match="adj must have shape"):
        gmpe.gnn_base(x, z(10, 6, 5), ids, ok())
    with pytest.raises(ValueError, match="adj must have shape"):
        gmpe.gnn_base(x, z(3, 6, 6), ids, ok())          # 10 rows are no multiple of 3 matrices
    with pytest.raises(ValueError, match="agent_id must have shape"):
        gmpe.gnn_base(x, adj, z(9, dtype=torch.int64), ok())
    with pytest.raises(ValueError, match=r"lin1.weight must have shape \(16, 10\)"):
        gmpe.gnn_base(z(10, 6, 8), adj, ids, ok())
    with pytest.raises(ValueError, match="base must have .gnn"):
        gmpe.gnn_base(x, adj, ids, types.SimpleNamespace())
    bad = ok()
    bad.gnn.graph_aggr = "all"
    with pytest.raises(ValueError, match="graph_aggr = 'all'"):
        gmpe.gnn_base(x, adj, ids, bad)
    bad = ok(aggr="mean")
    bad.gnn.global_aggr_type = "min"
    with pytest.raises(ValueError, match="global_aggr_type = 'min'"):
        gmpe.gnn_base(x, adj, ids, bad)
    bad = ok()
    bad.gnn.gnn1.lin_edge = torch.nn.Linear(1, 48)
    with pytest.raises(ValueError, match="lin_edge has a bias"):
        gmpe.gnn_base(x, adj, ids, bad)
    bad = ok()
    del bad.gnn.gnn1.lin_skip
    with pytest.raises(ValueError, match=r"gnn1\.lin_skip is missing"):
        gmpe.gnn_base(x, adj, ids, bad)
    # everything else in order: the arrays are not on a device. embed_add_self_loop is inert, either value; the compact adjacency; ids as [rows, 1] floats
    for base in (ok(), G.build(cfg), G.build(G.CONFIGS[G.CRITIC]), ok(ln=0, embed_n=0, gnn_n=0, heads=1, eact="Tanh", cact="Tanh", aggr="max")):
        base.gnn.embed_layer._add_self_loops = True
        with pytest.raises(ValueError, match="no CPU fallback"):
            gmpe.gnn_base(x, adj[::5], ids.view(10, 1).float(), base)


# ---------------------------------------------------------------------------------------------- (c)
def test_no_kernel_of_the_file_uses_scratch_memory():
    assert "gnn" in abi_lib.ru_objects()                                                            # `make resource-usage` holds it
    names, scratch = list(abi_lib.kernels("gnn")), list(abi_lib.scratch("gnn", "k_gnn").values())
    assert len(names) == len(scratch) == 4 and all(s == 0 for s in scratch), (names, scratch)       # forward, the two backward halves, finish
    for k in ("k_gnn_fwd", "k_gnn_bwd_conv", "k_gnn_bwd_embed", "k_gnn_finish"):
        assert any(k in n for n in names), k
