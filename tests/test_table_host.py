"""tests/table_lib.py (the entity table restated in NumPy, the truth of tests/test_gpu_table_consumers.py) against the oracle, without a device: the mask
words a step writes for done agents are the bits status and goal_tracker imply, in every word; the restated adjacency has the oracle's zero pattern; the
restated rows and adjacency agree with the oracle's step outputs at the tolerance the project holds expanded rows to (atol 1e-5, tests/test_gpu_gather.py).
All four row kinds at A = 33 (E = 66, three mask words) and navigation_graph at A = 64 (E = 128, four). And synthetic()'s own invariants, and the committed
seeds of the GNN cases: each keeps gnn_lib.MARGIN in every graph."""
import functools

import numpy as np
import pytest

import gmpe
import gnn_lib as G
import oracle_lib as ol
import table_lib as TL

CASES = {"relative_E66": (dict(scenario_name=TL.NAV), 33, 8.0, 0, 0, 8), "global_E66": (dict(scenario_name=TL.NAV, graph_feat_type="global"), 33, 8.0, 2, 0, 7),
         "rot_inv_E66": (dict(scenario_name=TL.ROT), 33, 8.0, 1, 0, 7), "two_phase_E66": (dict(scenario_name=TL.TWO), 33, 8.0, 1, 1, 7),
         "relative_E128": (dict(scenario_name=TL.NAV), 64, 12.0, 0, 0, 8)}
FIRST_DONE = 20


@functools.lru_cache(maxsize=None)
def stepped(key):
    """reset, agents 20.. forced done, one step of the oracle -> (cfg, table [N, W], node_obs [N, A, E, F] f64, adj [N, E, E] f64, the mask [N, E] that
    status and goal_tracker imply after the step: node i of a done agent and node A + goal_tracker[i])"""
    kw, A, side, kind, two, F = CASES[key]
    cfg = gmpe.make_config(num_envs=3, num_agents=A, world_size=side, episode_length=25, seed=61, **kw)
    assert TL.row_kind(cfg) == (kind, two) and cfg.node_feats == F and cfg.num_entities == 2 * A
    orc = ol.Oracle(cfg)
    orc.reset()
    TL.force_done(orc, np.arange(FIRST_DONE, A))
    rng = np.random.RandomState(3)
    out = orc.step(rng.randint(0, cfg.n_actions, (cfg.num_envs, A)).astype(np.int32))
    assert not out[7].any()                                  # no env has reset
    st, gt = orc.get("status").astype(bool), orc.get("goal_tracker")
    implied = np.zeros((cfg.num_envs, 2 * A), dtype=bool)
    for n, i in zip(*np.nonzero(st)):
        implied[n, i] = implied[n, A + gt[n, i]] = True
    assert st[:, FIRST_DONE:].all() and np.array_equal(gt[:, FIRST_DONE:], np.broadcast_to(np.arange(FIRST_DONE, A), (cfg.num_envs, A - FIRST_DONE)))
    return cfg, orc.entity_table(), out[2], out[3], implied


@pytest.mark.parametrize("key", sorted(CASES))
def test_mask_words_are_the_bits_status_and_goal_tracker_imply(key):
    cfg, table, _, _, implied = stepped(key)
    A, E = cfg.num_agents, cfg.num_entities
    lay = TL.layout(cfg)
    words = table[:, lay["mask"]:]
    assert words.shape[1] == lay["words"] == (E + 31) // 32 and lay["width"] == table.shape[1]
    want = TL.words_of(TL.implied_mask(cfg, np.arange(FIRST_DONE, A)))
    if E == 66:                                              # agents 20 .. 32 and landmarks 53 .. 65, written out
        bits = lambda lo, hi: sum(1 << b for b in range(lo, hi + 1))
        assert want.tolist() == [bits(20, 31), 1 | bits(21, 31), 3]
    else:
        assert want.tolist() == [sum(1 << b for b in range(20, 32)), 0xFFFFFFFF, sum(1 << b for b in range(20, 32)), 0xFFFFFFFF]
    forced_only = (implied == TL.implied_mask(cfg, np.arange(FIRST_DONE, A))).all(1)      # an agent below 20 may reach its goal in this step on its own
    assert forced_only.sum() >= 2
    assert np.array_equal(words[forced_only], np.broadcast_to(want.astype(np.float64), (int(forced_only.sum()), lay["words"])))
    assert np.array_equal(words, TL.words_of(implied).astype(np.float64)) and np.array_equal(TL.mask_bits(cfg, table), implied)


@pytest.mark.parametrize("key", sorted(CASES))
def test_the_restatement_agrees_with_the_oracles_step_outputs(key):
    cfg, table, node, adj, _ = stepped(key)
    rows, a, masked = TL.rows_and_adj(cfg, table)
    assert rows.dtype == np.float32 and a.dtype == np.float32 and rows.shape == node.shape and a.shape == adj.shape
    assert np.array_equal(a == 0, adj == 0), "the zero pattern of the adjacency"
    assert masked.any() and not masked.all() and (a[masked] == 0).all() and (a.transpose(0, 2, 1)[masked] == 0).all()
    assert (a[:, 0, 1:FIRST_DONE] > 0).any()
    print(key, "rows", float(np.abs(rows - node).max()), "adj", float(np.abs(a - adj).max()))
    np.testing.assert_allclose(rows, node, rtol=0, atol=1e-5)
    np.testing.assert_allclose(a, adj, rtol=0, atol=1e-5)


def test_the_layout_follows_the_documented_width():
    for E in TL.SHAPES:
        for kind in TL.KINDS:
            cfg = TL.config(E, kind)
            lay = TL.layout(cfg)
            A = cfg.num_agents
            assert cfg.num_entities == E and lay["width"] == cfg.entity_table_width and lay["words"] == (E + 31) // 32
            assert (lay["x"], lay["y"], lay["vox"], lay["voy"], lay["vnx"], lay["vny"]) == (0, E, 2 * E, 2 * E + A, 2 * E + 2 * A, 2 * E + 3 * A)
            assert (lay["cos"] is not None) == (kind in (1, "two")) and (lay["exit"] is not None) == (kind == "two")
            if kind == "two":
                assert lay["exit"] == lay["mask"] - 2 == lay["sin"] + A


@pytest.mark.parametrize("E", sorted(TL.SHAPES))
def test_synthetic_tables_keep_their_invariants(E):
    cfg = TL.config(E, "two")
    names, tables, masked = TL.synthetic_patterns(cfg, seed=E, repeat=2)
    lay = TL.layout(cfg)
    assert set(names) == set(TL.PATTERNS) - ({"node 64"} if E <= 64 else set()) and tables.shape == (len(names), lay["width"])
    words = tables[:, lay["mask"]:]
    assert np.array_equal(words, np.floor(words)) and (words >= 0).all() and (words < 2.0 ** 32).all()
    if E % 32:                                               # no bit at or above E in the last word
        assert (words[:, -1] < 2.0 ** (E % 32)).all()
    assert np.array_equal(TL.mask_bits(cfg, tables), masked)  # masked is recovered from the words
    by = dict(zip(names[:len(names) // 2], masked))
    assert not by["none"].any() and by["everything"].all() and by["a random half"].sum() == E // 2
    assert np.flatnonzero(by["node 0"]).tolist() == [0] and np.flatnonzero(by["node E - 1"]).tolist() == [E - 1] and np.flatnonzero(by["node 32"]).tolist() == [32]
    assert np.flatnonzero(by["bit 31 of every word"]).tolist() == list(range(31, E, 32))
    if E > 64:
        assert np.flatnonzero(by["node 64"]).tolist() == [64]
    # positions in the world, unit headings, vn != vo for some agents and equal for others, two draws of a pattern differ
    A = cfg.num_agents
    half = cfg.world_size / 2
    assert (np.abs(tables[:, :2 * E]) <= half).all()
    assert np.allclose(tables[:, lay["cos"]:lay["cos"] + A] ** 2 + tables[:, lay["sin"]:lay["sin"] + A] ** 2, 1.0)
    same = tables[:, lay["vox"]:lay["vox"] + A] == tables[:, lay["vnx"]:lay["vnx"] + A]
    assert same[:, 0::2].all() and not same[:, 1::2].any()
    assert not np.array_equal(tables[0, :2 * E], tables[len(names) // 2, :2 * E])
    rows, adj, m = TL.rows_and_adj(cfg, tables)
    assert np.array_equal(m, masked) and np.isfinite(rows).all() and (adj[names.index("everything")] == 0).all()
    edges = (adj[0] > 0) & (adj[0] < G.MAX_EDGE_DIST)
    assert 4 <= edges.sum() / E <= 20                        # about ten neighbours within max_edge_dist: the GNN tests have edges and non-edges


def test_the_restatement_is_sensitive_to_what_the_mutants_change():
    """what separates a right consumer from one that reads word 0 for every node, shifts by r & 15, or ignores the column's bit"""
    cfg = TL.config(66, 0)
    names, tables, masked = TL.synthetic_patterns(cfg, seed=1)
    _, adj, _ = TL.rows_and_adj(cfg, tables)
    i = names.index("node 64")
    assert (adj[i, 64] == 0).all() and (adj[i, :, 64] == 0).all() and (adj[i, 0, 1:64] > 0).all() and (adj[i, 32, :32] > 0).all()
    i = names.index("node 32")
    assert (adj[i, 32] == 0).all() and (adj[i, :, 32] == 0).all() and (adj[i, 0, 1:32] > 0).all() and (adj[i, 64, :32] > 0).all()
    i = names.index("bit 31 of every word")
    assert (adj[i, 31] == 0).all() and (adj[i, 63] == 0).all() and (adj[i, 15, :15] > 0).all() and (adj[i, 47, :15] > 0).all()


@pytest.mark.parametrize("E", sorted(TL.SHAPES))
def test_every_gnn_case_has_a_committed_seed_that_keeps_the_relu_margin(E):
    """no graph of a GNN case of tests/test_gpu_table_consumers.py is dropped or redrawn at run time: the committed seed keeps gnn_lib.MARGIN in every graph,
    and the float32 CPU run of the restatement stays under the cap of the accuracy rule"""
    for kind, weights in TL.GNN_WEIGHTS:
        case = TL.gnn_case(E, kind, weights)
        n = len(case["names"])
        assert case["x"].shape == (2 * n + 1, E, case["cfg"].node_feats) and case["adj"].shape == (2 * n + 1, E, E) and n == (8 if E > 64 else 7)
        m = TL.gnn_margins(case)
        assert m.shape == (2 * n + 1,) and (m >= G.MARGIN).all(), (E, kind, weights, float(m.min()))
        t, e_ref = TL.gnn_truth(case)
        assert np.isfinite(t).all() and e_ref <= G.CAP, (E, kind, weights, e_ref)
        edges = (case["adj"] > 0) & (case["adj"] < G.MAX_EDGE_DIST)
        assert edges.any() and not edges[case["names"].index("everything")].any()
