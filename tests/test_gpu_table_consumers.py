"""Every consumer of the fp64 entity table against tests/table_lib.py, the table restated in NumPy (tests/test_table_host.py holds it to the oracle), past the
first mask word: E = 33, 64, 65, 66, 97 and 128, every row kind, and mask bits in every word.
  - the writer: the engine's table is the oracle's, mask words exactly, after agents were forced done so that words 1 .. 3 have bits; the engine's own
    node_obs and adj are the restatement of its own table;
  - gmpe_expand_node_obs / gmpe_expand_adj, the table kinds of gmpe_minibatch_gather, the GMPE_MBE_TABLE source of gmpe_minibatch_edges, and the table
    source of the narrow and of the wide GNN kernel on synthetic tables (table_lib.synthetic: every required mask pattern).
Every comparison is bit for bit (array_equal / torch.equal); the GNN kernels are compared with the same kernel on the restated rows and adjacency, and
their features are held to tests/gnn_lib.py's float64 restatement under the project's rule (err_dev <= 4 * err_ref + 2^-23, err_ref <= 1e-5)."""
import functools

import numpy as np
import pytest
import torch

import gmpe
import gnn_lib as G
import mb_edges_lib as EL
import minibatch_lib as M
import oracle_lib as ol
import table_lib as TL
from gmpe import _lib, gnn as W
from test_gpu_minibatch_kernel import _gather, _same_image

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL_E = sorted(TL.SHAPES)
KIND_IDS = {0: "relative", 1: "rot_inv", "two": "two_phase", 2: "global"}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        raise AssertionError("%s: %d of %d elements differ, first at %s: %r != %r" % (what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])],
                                                                                        want[tuple(bad[0])]))


# ---------------------------------------------------------------------------------------------- the writer
WRITER = [(33, 0), (65, 0), (66, 0), (66, 1), (66, "two"), (66, 2), (128, 0)]


@pytest.mark.parametrize("E,kind", WRITER, ids=["E%d_%s" % (E, KIND_IDS[k]) for E, k in WRITER])
def test_the_engine_writes_the_oracles_table_and_its_own_rows_are_the_restatement(E, kind):
    from gmpe.engine import GmpeEngine
    cfg = TL.config(E, kind, num_envs=2, world_size=12.0 if E > 66 else 8.0, episode_length=25, seed=71)
    A = cfg.num_agents
    eng, orc = GmpeEngine(cfg, node_form="both", adj_compact=True), ol.Oracle(cfg)
    eng.reset(); orc.reset()
    done = np.arange(min(20, A - 5), A)
    TL.force_done(eng, done); TL.force_done(orc, done)
    act = np.random.RandomState(5).randint(0, cfg.n_actions, (2, A)).astype(np.int32)
    o = eng.step(torch.as_tensor(act)); oo = orc.step(act)
    eng.check_errors()
    assert not oo[7].any()
    tab, tab_o = o.entity_table.cpu().numpy(), orc.entity_table()
    lay = TL.layout(cfg)
    np.testing.assert_allclose(tab, tab_o, rtol=0, atol=1e-9)
    assert np.array_equal(tab[:, lay["mask"]:], tab_o[:, lay["mask"]:]), "mask words"
    masked = TL.mask_bits(cfg, tab)
    want = TL.implied_mask(cfg, done)
    assert (masked[:, want]).all() and masked.sum() <= 2 * (want.sum() + 4)           # the forced agents, and at most a few that arrived on their own
    has_bit = TL.words_of(want) != 0                                                  # every word past the first that holds an agent or a landmark has bits
    assert ((tab[:, lay["mask"]:] != 0) | ~has_bit).all() and has_bit[1:].sum() == {33: 0, 65: 1, 66: 2, 128: 3}[E]
    rows, adj, _ = TL.rows_and_adj(cfg, tab)
    same_bits(o.node_obs, rows, "the engine's node_obs")
    same_bits(o.adj, adj, "the engine's adj")
    np.testing.assert_allclose(rows, oo[2], rtol=0, atol=1e-5)


# ---------------------------------------------------------------------------------------------- gmpe_expand_node_obs / gmpe_expand_adj
@pytest.mark.parametrize("kind", list(TL.KINDS), ids=list(KIND_IDS.values()))
@pytest.mark.parametrize("E", ALL_E)
def test_expand_node_obs_and_expand_adj_on_every_mask_pattern(E, kind):
    from gmpe.engine import expand_adj, expand_node_obs
    cfg = TL.config(E, kind)
    names, tables, masked = TL.synthetic_patterns(cfg, seed=300 + E)
    rows, adj, m = TL.rows_and_adj(cfg, tables)
    assert np.array_equal(m, masked) and (E * E % 4 != 0) == (E % 2 == 1)
    t = dev(tables)
    same_bits(expand_node_obs(cfg, t), rows, "expand_node_obs")
    same_bits(expand_adj(cfg, t), adj, "expand_adj")
    if kind in (0, "two"):                                   # the materialised per-agent form, and blocks written into a larger array at an env offset
        A, n = cfg.num_agents, len(names)
        same_bits(expand_adj(cfg, t, copies=A), np.ascontiguousarray(np.broadcast_to(adj[:, None], (n, A, E, E))), "expand_adj copies=A")
        blocks = t.view(2, n // 2, -1) if n % 2 == 0 else t[:n - 1].reshape(2, n // 2, -1).contiguous()
        nb = blocks.shape[1]
        for fn, truth, tail in ((expand_node_obs, rows, rows.shape[1:]), (expand_adj, adj, adj.shape[1:])):
            big = torch.full((2, nb + 3) + tuple(tail), -7.0, device=DEV)
            fn(cfg, blocks, out=big, out_envs=nb + 3, env_offset=2)
            same_bits(big[:, 2:2 + nb].contiguous(), truth[:2 * nb].reshape((2, nb) + tuple(tail)), fn.__name__ + " at an env offset")
            assert bool((big[:, :2] == -7.0).all()) and bool((big[:, 2 + nb:] == -7.0).all())


# ---------------------------------------------------------------------------------------------- the minibatch gather's table kinds, the edge lists
MB_T, MB_N = 3, 2
SLOT_ORDER = ("bit 31 of every word", "node E - 1", "node 32", "node 64", "a random half", "everything", "none", "node 0")


@functools.lru_cache(maxsize=None)
def slots(E, kind):
    """synthetic slot tables [T + 1, N, W], the mask patterns spread over the slots -> (cfg, tables, node_obs [T+1, N, A, E, F], adj [T+1, N, E, E])"""
    cfg = TL.config(E, kind, num_envs=MB_N)
    names, tables, _ = TL.synthetic_patterns(cfg, seed=500 + E)
    assert len(names) == (MB_T + 1) * MB_N == 8
    order = [names.index(n) for n in SLOT_ORDER]             # a minibatch draws from slots 0 .. T - 1: the last slot holds the two plainest patterns
    tables = tables[order].reshape(MB_T + 1, MB_N, -1)
    rows, adj, _ = TL.rows_and_adj(cfg, tables)
    return cfg, tables, rows, adj


def mb_case(E, kind, recurrent, fields, seed):
    """fields: ("node" | "adj", pad, dst_off) -> (cfg, plan, image before, image expected): the sources are the slot tables, slot_stride apart, the
    expected rows are the restatement's; destinations and guards hold the sentinel"""
    cfg, tables, node, adj = slots(E, kind)
    T, N, A, F, Wd = MB_T, MB_N, cfg.num_agents, cfg.node_feats, cfg.entity_table_width
    spec = dict(node=(_lib.MB_TABLE_NODE, E * F * 4), adj=(_lib.MB_TABLE_ADJ, E * E * 4))
    L = 7 if recurrent else 1
    n_valid = T * N * A // L
    rng = np.random.RandomState(seed)
    entries = rng.randint(0, n_valid, 9 if recurrent else 23).astype(np.int64)
    entries[[1, 3, 4]] = (-1, 2 ** 32 + 3, n_valid)          # out of range, among valid and duplicated entries
    rows, off = len(entries), 3
    laid, src0, size = M.layout(T, N, A, lambda k: rows * L, [(spec[k][0], spec[k][1], pad, 0, do) for k, pad, do in fields], table_row=Wd * 8)
    perm = rng.randint(0, n_valid, off + max(rows, L) + 3).astype(np.int64)
    perm[off:off + rows] = entries
    plan = dict(mode=M.RECURRENT if recurrent else M.FEED_FORWARD, T=T, N=N, A=A, L=L, perm=perm, offset=off, rows=rows, fields=laid, src0=src0)
    image = np.full(size, M.SENTINEL, dtype=np.uint8)
    image[src0:] = M.source_bytes(seed + 1, size - src0)
    for f in laid:
        for t in range(T + 1):
            b = np.ascontiguousarray(tables[t]).reshape(-1).view(np.uint8)
            image[f["src"] + t * f["slot_stride"]:f["src"] + t * f["slot_stride"] + b.size] = b
    want = image.copy()
    ok, t, n, a = M.row_samples(plan)
    assert ok.sum() == (rows - 3) * L and len(set(zip(t[ok], n[ok]))) >= (4 if recurrent else 6)    # the slots drawn, each with its mask pattern
    for f, (k, pad, do) in zip(laid, fields):
        rb = f["row_bytes"]
        for r in np.flatnonzero(ok):
            row = node[t[r], n[r], a[r]] if k == "node" else adj[t[r], n[r]]
            want[f["dst"] + r * rb:f["dst"] + (r + 1) * rb] = np.ascontiguousarray(row).reshape(-1).view(np.uint8)
    return cfg, plan, image, want


@pytest.mark.parametrize("recurrent", [False, True], ids=["ff", "rec"])
@pytest.mark.parametrize("kind", list(TL.KINDS), ids=list(KIND_IDS.values()))
@pytest.mark.parametrize("E", [65, 66])
def test_minibatch_gather_table_kinds_at_three_mask_words(E, kind, recurrent):
    """E = 65: one entry per thread; E = 66: four (E * E % 4 == 0) where the destination allows it, one where an adj destination is 4 bytes off"""
    assert (E * E % 4 == 0) == (E == 66)
    plans = {"aligned": [("node", 0, 0), ("adj", 0, 0)], "adj 4 bytes off, slot + 8 bytes": [("adj", 8, 4), ("node", 8, 0)]}
    for i, (what, fields) in enumerate(plans.items()):
        cfg, plan, image, want = mb_case(E, kind, recurrent, fields, 700 + 10 * E + i)
        assert not np.array_equal(want, image)
        _same_image(_gather(torch, plan, image, cfg), want, plan, (E, kind, what))


@pytest.mark.parametrize("L", [None, 7], ids=["ff", "rec"])
@pytest.mark.parametrize("kind", [0, "two"], ids=["relative", "two_phase"])
@pytest.mark.parametrize("E", [65, 66])
def test_minibatch_edges_from_the_table_at_three_mask_words(E, kind, L):
    """the edge list is NumPy's nonzero over the restated, thresholded adjacency (the adjacency does not depend on the row kind: two table widths)"""
    from gmpe.minibatch import edge_list
    cfg, tables, _, adj = slots(E, kind)
    T, N, A = MB_T, MB_N, cfg.num_agents
    adj5 = np.broadcast_to(adj[:, :, None], (T + 1, N, A, E, E))
    n_valid = T * N * A if L is None else T * N * A // L
    rows, off = (61, 3) if L is None else (9, 2)
    perm = EL.synthetic_perm(rows, n_valid, seed=E + (L or 0), extra=off + 4)
    perm[off + 2], perm[off + 5] = -1, n_valid                                     # graphs without edges among the others
    t, n, _, ok = EL.samples(perm, off, rows, T, N, A, L)
    assert len(set(zip(t[ok], n[ok]))) >= 5                                        # most slots, so most mask patterns, are drawn
    src, perm_d = dev(tables), dev(perm)
    for inclusive, index64 in ((False, True), (True, False)):
        ei, ea, counts = EL.minibatch_edges(adj5, perm, off, rows, T, N, A, 1.0, L, inclusive=inclusive, dtype=np.int64 if index64 else np.int32)
        assert (counts == 0).sum() >= 2 and (counts > 0).sum() >= 5 and ei.shape[1] > E
        el = edge_list(cfg, torch.device(DEV), _lib.MBE_TABLE, src, T, N, A, E, 1.0, perm=perm_d, offset=off, rows=rows, data_chunk_length=L,
                       inclusive=inclusive, index64=index64)
        got_i, got_a = el.edge_index.cpu().numpy(), el.edge_attr.cpu().numpy()
        assert el.n_edges == ei.shape[1] and got_i.dtype == ei.dtype and np.array_equal(got_i, ei), (E, kind, L, inclusive)
        same_bits(got_a, ea, "edge_attr")


# ---------------------------------------------------------------------------------------------- the GNN kernels' table source
@functools.lru_cache(maxsize=None)
def device_base(key):
    return G.build(G.CONFIGS[key]).to(DEV)


def on_device(case, dtype=torch.int64):
    return dev(case["tables"]), dev(case["idx"]).to(dtype), dev(case["ego"]), dev(case["x"]), dev(case["adj"])


def held_to_float64(case, got, what):
    t64, e_ref = TL.gnn_truth(case)
    e_dev = G.err(got.cpu().numpy(), t64)
    print("%s features err_ref %.3g err_dev %.3g bound %.3g" % (what, e_ref, e_dev, G.bound(e_ref)))
    assert e_ref <= G.CAP, (what, e_ref)
    assert e_dev <= G.bound(e_ref), (what, e_dev, e_ref)


def grads_of(f, base, gf):
    return [f.detach()] + list(torch.autograd.grad((f * gf).sum(), list(base.parameters())))


GNN_IDS = ["%s_%s" % (KIND_IDS[k], w.lower()) for k, w in TL.GNN_WEIGHTS]


@pytest.mark.parametrize("kind,weights", TL.GNN_WEIGHTS, ids=GNN_IDS)
@pytest.mark.parametrize("E", [33, 64])
def test_narrow_gnn_from_the_table_is_gnn_base_on_the_restated_rows(E, kind, weights):
    """features and every gradient, bit for bit; E = 64 takes its gradients through the actor's gather (the critic's there are the mean pool's, whose
    float32 reference breaks the cap, tests/gnn_lib.py) — here gradients are compared in bits only, so both run"""
    case = TL.gnn_case(E, kind, weights)
    cfg, base = case["cfg"], device_base(case["key"])
    tabs, idx, ego, x, a = on_device(case)
    gf = torch.randn((len(case["idx"]), G.C), generator=torch.Generator().manual_seed(E)).to(DEV)
    got = grads_of(gmpe.gnn_base_from_table(tabs, idx, ego, base, cfg), base, gf)
    want = grads_of(gmpe.gnn_base(x, a, ego, base), base, gf)
    assert len(got) == len(want) == 1 + len(list(base.parameters()))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and torch.equal(g, w), "%s differs" % ("features" if i == 0 else "gradient %d" % (i - 1))
    assert bool(torch.isfinite(got[0]).all()) and float(got[0].abs().max()) > 0 and any(float(g.abs().max()) > 0 for g in got[1:])
    with torch.no_grad():
        assert torch.equal(gmpe.gnn_base_from_table(tabs, idx.to(torch.int32), ego, base, cfg), want[0])
    assert torch.equal(got[0][-1], got[0][0])                # the repeated graph
    held_to_float64(case, got[0], "narrow E=%d %s %s" % (E, kind, weights))


def wide_pair(case, base, dtype=torch.int64):
    tabs, idx, ego, x, a = on_device(case, dtype)
    with torch.no_grad():
        return gmpe.gnn_base_wide_from_table(tabs, idx, ego, base, case["cfg"]), gmpe.gnn_base_wide(x, a, ego, base)


@pytest.mark.parametrize("kind,weights", TL.GNN_WEIGHTS, ids=GNN_IDS)
@pytest.mark.parametrize("E", [65, 66, 97, 128])
def test_wide_gnn_from_the_table_is_gnn_base_wide_on_the_restated_rows(E, kind, weights):
    case = TL.gnn_case(E, kind, weights)
    cfg, base = case["cfg"], device_base(case["key"])
    assert W.wide_geometry(len(case["idx"]), E, cfg.node_feats)[0] == (2 if E < 90 else 1)
    got, want = wide_pair(case, base)
    assert got.shape == (len(case["idx"]), G.C) and torch.equal(got, want), "features differ"
    assert torch.equal(wide_pair(case, base, torch.int32)[0], want) and torch.equal(got[-1], got[0])
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
    held_to_float64(case, got, "wide E=%d %s %s" % (E, kind, weights))
    # everything masked: no edge at all, so every ego gives the same finite row
    names, n = case["names"], len(case["names"])
    i = names.index("everything")
    tabs = dev(case["tables"])
    egos = torch.tensor([0, 1, cfg.num_agents // 2, cfg.num_agents - 1], device=DEV)
    with torch.no_grad():
        f = gmpe.gnn_base_wide_from_table(tabs, torch.full((4,), i, device=DEV), egos, base, cfg)
    assert bool(torch.isfinite(f).all()) and torch.equal(f, f[:1].expand(4, G.C)) and torch.equal(f[0], got[i]) and torch.equal(f[0], got[n + i])
    # node 64 only: the unmasked table with that one bit set gives other features to the graph of node 64's nearest agent
    lay = TL.layout(cfg)
    pair = np.stack([case["tables"][names.index("none")]] * 2)
    assert (pair[:, lay["mask"]:] == 0).all()
    pair[1, lay["mask"] + 2] = 1.0
    _, adj, m = TL.rows_and_adj(cfg, pair)
    assert np.flatnonzero(m[1]).tolist() == [64] and not m[0].any()
    near = int(np.argmin(adj[0, 64, :cfg.num_agents]))       # the agent nearest to node 64: an edge in the unmasked table, none in the other
    assert 0 < adj[0, 64, near] < G.MAX_EDGE_DIST and adj[1, 64, near] == 0 and near != 64
    rows = TL.rows_and_adj(cfg, pair)[0]
    ego = torch.tensor([near, near], device=DEV)
    with torch.no_grad():
        f = gmpe.gnn_base_wide_from_table(dev(pair), torch.tensor([0, 1], device=DEV), ego, base, cfg)
        assert not torch.equal(f[0], f[1]) and torch.equal(f, gmpe.gnn_base_wide(dev(rows[:, near]), dev(adj), ego, base))


SHARE = [(65, 0, "ROTATE"), (66, 1, "CRITIC"), (97, "two", "ACTOR"), (128, 2, "ACTOR")]


@pytest.mark.parametrize("E,kind,weights", SHARE, ids=["E%d_%s_%s" % (E, KIND_IDS[k], w.lower()) for E, k, w in SHARE])
def test_wide_gnn_table_share_form_on_every_ego_of_every_pattern(E, kind, weights):
    """table_index None, table_share = A: table n serves its A graphs, against the compact adjacency of gnn_base_wide"""
    case = TL.gnn_case(E, kind, weights)
    cfg, base = case["cfg"], device_base(case["key"])
    A, n = cfg.num_agents, len(case["names"])
    rows, adj, _ = TL.rows_and_adj(cfg, case["tables"])
    egos = torch.arange(A, device=DEV).repeat(n)
    with torch.no_grad():
        got = gmpe.gnn_base_wide_from_table(dev(case["tables"]), None, egos, base, cfg, table_share=A)
        want = gmpe.gnn_base_wide(dev(rows.reshape(n * A, E, -1)), dev(adj), egos, base)
        assert got.shape == (n * A, G.C) and torch.equal(got, want)
        # the indexed call's graphs are among them
        flat = torch.as_tensor(case["idx"] * A + case["ego"], device=DEV)
        assert torch.equal(got[flat], wide_pair(case, base)[0])


def test_wide_gnn_from_the_table_on_a_workgroup_that_owns_two_tiles():
    """E = 65 at the shipped sizes: W = 2 on 256 workgroups, so 527 graphs are 264 tiles and workgroups 0 .. 7 own two. 31 repetitions of the 17-graph
    case: every repetition has the small call's bits"""
    case = TL.gnn_case(65, 1, "ACTOR")
    base = device_base(case["key"])
    r = len(case["idx"])
    Wg, lds, blocks = W.wide_geometry(31 * r, 65, 7)
    assert r == 17 and (Wg, blocks) == (2, 256) and (31 * r + Wg - 1) // Wg > blocks
    small, want = wide_pair(case, base)
    assert torch.equal(small, want)
    tabs, idx, ego, _, _ = on_device(case)
    with torch.no_grad():
        big = gmpe.gnn_base_wide_from_table(tabs, idx.repeat(31), ego.repeat(31), base, case["cfg"])
    assert big.shape == (31 * r, G.C) and torch.equal(big.view(31, r, G.C), small.expand(31, r, G.C))
