"""The GNNBase forward on graphs of 65 .. 128 nodes (gmpe.gnn_base_wide, gmpe.gnn_base_wide_from_table, gmpe_gnn_forward_wide / _wide_table).
  - accuracy: against the float64 restatement of tests/gnn_lib.py, the project's rule on `features`: err_dev <= 4 * err_ref + 2^-23, err_ref <= 1e-5;
  - bits: a graph of <= 64 nodes padded with isolated nodes keeps gmpe.gnn_base's row in the ego (no tolerance: this ties the wide kernel to the narrow
    one); E <= 64 through the wide entries is the narrow entries' result; a graph does not depend on its batch, its place, the number of graphs side by
    side or the adjacency's form; the table source gives the bits of the rows and adjacency the same engine wrote;
  - the C entries on a side stream between guard bytes; collect_step / compute / evaluator_act / CapturedRollout at A = 33 agents (E = 66)."""
import copy
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

import gmpe
import gnn_lib as G
from gmpe import _lib, gnn as W, policy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R = G._RANDOM
LARGEST, TANH_ADD, TANH_RELU = G.cfg_key(R[-1]), G.cfg_key(R[5]), G.cfg_key(R[6])
# (graphs, E, configuration, special graphs): E = 84 and 85 inside W = 2, both sides of W = 2 | 1 (87 | 88 at the shipped sizes, 81 | 82 at the largest
# configuration: BOUNDARY below, the fullest LDS the kernel gets), E = 65 and 128, every aggregate, the largest configuration gnn_base accepts at W = 1
# (E = 100, 128), Tanh, and the written edge cases at E = 70
BOUNDARY = ((4, 87, G.ACTOR, False), (4, 88, G.ACTOR, False), (4, 81, LARGEST, False), (4, 82, LARGEST, False))
CASES = ((5, 65, G.ACTOR, False), (5, 65, G.CRITIC, False), (5, 65, G.ROTATE, False), (4, 84, G.ACTOR, False), (4, 85, G.ACTOR, False)) + BOUNDARY + (
         (6, 96, G.ACTOR, False), (6, 96, G.CRITIC, False), (9, 128, G.ACTOR, False), (9, 128, G.CRITIC, False), (9, 128, G.ACTOR_MAX, False),
         (9, 128, G.ACTOR_ADD, False), (6, 100, LARGEST, False), (3, 128, LARGEST, False), (6, 90, TANH_ADD, False), (6, 90, TANH_RELU, False),
         (8, 70, G.ACTOR, True), (8, 70, G.CRITIC, True))


def test_the_boundary_cases_lie_on_both_sides_of_two_graphs_per_workgroup():
    """W = 2, 1, 2, 1, and the two W = 2 launches ask for the most LDS of any: 162 496 and 162 336 of 163 840 bytes"""
    got = []
    for n, E, key, _ in BOUNDARY:
        c = G.CONFIGS[key]
        got.append(W.wide_geometry(n, E, c["F"], c["heads"], c["gnn_n"], c["embed_n"], c["nemb"], c["esz"])[:2])
    assert [g[0] for g in got] == [2, 1, 2, 1] and got[0][1] == 162496 and got[2][1] == 162336
    assert all(lds <= 160 * 1024 for _, lds in got)


@functools.lru_cache(maxsize=None)
def device_base(key):
    return G.build(G.CONFIGS[key]).to(DEV).requires_grad_(False)


def wide(key, x, adj, ids):
    with torch.no_grad():
        return gmpe.gnn_base_wide(x.to(DEV), adj.to(DEV), ids.to(DEV), device_base(key))


def narrow(key, x, adj, ids):
    with torch.no_grad():
        return gmpe.gnn_base(x.to(DEV), adj.to(DEV), ids.to(DEV), device_base(key))


@functools.lru_cache(maxsize=None)
def device_run(case):
    n, E, key, special = case
    x, adj, ids = G.inputs(n, E, key, special)[:3]
    return wide(key, x, adj, ids)


# ---------------------------------------------------------------------------------------------- accuracy
@pytest.mark.parametrize("case", CASES, ids=G.case_id)
def test_forward_agrees_with_the_float64_restatement(case):
    n, E, key, special = case
    t64, e_ref = G.truth(n, E, key, special)
    got = device_run(case).cpu().numpy()
    e_dev = G.err(got, t64["features"])
    print("%s features err_ref %.3g err_dev %.3g bound %.3g" % (G.case_id(case), e_ref["features"], e_dev, G.bound(e_ref["features"])))
    assert got.shape == (n, G.C) and np.isfinite(got).all()
    assert e_ref["features"] <= G.CAP, (case, e_ref["features"])
    assert e_dev <= G.bound(e_ref["features"]), (case, e_dev, e_ref["features"])


# ---------------------------------------------------------------------------------------------- padding: the tie to the narrow kernel
def padded(x, adj, ids, E, spread):
    """E0 -> E nodes: isolated ones (type 0, any finite features, adjacency rows and columns 0 or >= max_edge_dist) appended, or — spread — placed so
    that the original nodes keep their relative order but not their indices; the ego id follows its node"""
    n, E0, F = x.shape
    rng = np.random.RandomState(E0 * 1000 + E)
    keep = np.arange(E0) if not spread else np.sort(rng.permutation(E)[:E0])
    X = torch.from_numpy(rng.randn(n, E, F).astype(np.float32))
    X[:, :, F - 1] = 0.0
    A = torch.where(torch.from_numpy(rng.rand(n, E, E)) < 0.5, 0.0, G.MAX_EDGE_DIST + float(rng.rand())).float()
    A[:, torch.arange(E), torch.arange(E)] = 0.0
    k = torch.from_numpy(keep)
    X[:, k] = x
    A[:, k[:, None], k[None, :]] = adj
    return X, A, k[ids]


@pytest.mark.parametrize("spread", [False, True], ids=["appended", "spread"])
@pytest.mark.parametrize("E0,E", [(6, 65), (20, 100), (64, 65), (64, 128), (44, 85), (64, 87)])
def test_a_padded_graph_keeps_gnn_bases_bits(E0, E, spread):
    x, adj, ids = G.inputs(5, E0, G.ACTOR)[:3]
    X, A, I = padded(x, adj, ids, E, spread)
    mask = (A > 0) & (A < G.MAX_EDGE_DIST)
    assert int(mask.sum()) == int(((adj > 0) & (adj < G.MAX_EDGE_DIST)).sum()) and X.shape == (5, E, 7)      # the padding adds no edge
    want, got = narrow(G.ACTOR, x, adj, ids), wide(G.ACTOR, X, A, I)
    assert float(want.abs().max()) > 0 and torch.equal(got, want)


# ---------------------------------------------------------------------------------------------- E <= 64 through the wide entries
@pytest.mark.parametrize("key", [G.ACTOR, G.CRITIC, G.ACTOR_MAX, G.ACTOR_ADD])
@pytest.mark.parametrize("n,E", [(65, 7), (12, 64)])
def test_up_to_64_nodes_the_wide_entries_are_the_narrow_ones(n, E, key):
    x, adj, ids = G.inputs(n, E, G.ACTOR)[:3]           # one draw for the four aggregates
    want = narrow(key, x, adj, ids)
    assert torch.equal(wide(key, x, adj, ids), want) and float(want.abs().max()) > 0


# ---------------------------------------------------------------------------------------------- independence from the batch
@pytest.mark.parametrize("case", [(5, 65, G.ACTOR, False), (9, 128, G.ACTOR, False), (9, 128, G.CRITIC, False)], ids=G.case_id)
def test_a_graph_does_not_depend_on_its_batch_or_its_place(case):
    n, E, key, _ = case                                 # n is odd: at W = 2 the last tile has an idle pair
    x, adj, ids = G.inputs(n, E, key)[:3]
    full = device_run(case)
    assert n % 2 == 1
    a = 0
    for m in (1, 2, 3):                                 # calls of 1, 2 and 3 graphs, so every graph changes its pair or its tile
        while a + m <= n:
            assert torch.equal(wide(key, x[a:a + m], adj[a:a + m], ids[a:a + m]), full[a:a + m]), "graphs %d .. %d" % (a, a + m - 1)
            a += m
        a = 0 if m < 3 else a
    assert torch.equal(wide(key, x.flip(0), adj.flip(0), ids.flip(0)).flip(0), full)
    for ids2 in (ids.to(torch.int32), ids.to(torch.float32), ids.view(n, 1)):       # the id's types and shapes
        assert torch.equal(wide(key, x, adj, ids2), full)


def test_a_workgroup_that_owns_two_tiles():
    """E = 65 at the shipped sizes: W = 2 on at most 256 workgroups, so 513 graphs are 257 tiles and workgroup 0 owns tiles 0 and 256. The batch is 57
    repetitions of a 9-graph one: every repetition has the small call's bits, whichever pair and tile its graphs fall on."""
    Wg, lds, blocks = W.wide_geometry(513, 65, 7)
    assert (Wg, blocks) == (2, 256) and (513 + Wg - 1) // Wg == blocks + 1
    x, adj, ids = G.inputs(9, 65, G.ACTOR)[:3]
    small = wide(G.ACTOR, x, adj, ids)
    big = wide(G.ACTOR, x.repeat(57, 1, 1), adj.repeat(57, 1, 1), ids.repeat(57))
    assert big.shape == (513, G.C) and torch.equal(big.view(57, 9, G.C), small.expand(57, 9, G.C))


@pytest.mark.parametrize("key", [G.ACTOR, G.CRITIC])
def test_the_compact_adjacency_gives_the_materialised_forms_bits(key):
    envs, S, E = 3, 33, 66
    x, _, _ = G.inputs(envs * S, E, key)[:3]
    adj = G.inputs(envs, E, key)[1]                     # one matrix per env, serving its S consecutive rows
    ids = torch.arange(S).repeat(envs)
    full = wide(key, x, adj.repeat_interleave(S, 0), ids)
    assert torch.equal(wide(key, x, adj, ids), full) and float(full.abs().max()) > 0


# ---------------------------------------------------------------------------------------------- edge cases
def test_the_written_edge_cases_and_clamped_types_and_ids_at_70_nodes():
    case = (8, 70, G.ACTOR, True)
    x, adj, ids = G.inputs(*case)[:3]
    mask = ((adj > 0) & (adj < G.MAX_EDGE_DIST)).numpy()
    assert not mask[0].any() and mask[1][:, 1].sum() == 1 and mask[2].sum() == 70 * 69 and not mask[3][1].any() and not mask[3][:, 1].any()
    assert adj[4, 0, 1] == G.MAX_EDGE_DIST and not mask[4][0, 1] and mask[4][1, 0] and mask[5][0, 1] and not np.tril(mask[5], -1).any()
    full = device_run(case)
    # no edge at all: every conv sees the skip alone, so the row is a function of the parameters — the same for every ego, finite
    for ego in (0, 63, 64, 69):
        one = wide(G.ACTOR, x[:1], adj[:1], torch.tensor([ego]))
        assert torch.equal(one, wide(G.ACTOR, x[:1], adj[:1], torch.tensor([0]))) and bool(torch.isfinite(one).all())
    # ids on both sides of the wave boundary and at the end, and clamped ones: below 0 is node 0, above E - 1 is node E - 1
    E = 128
    x2, adj2, _ = G.inputs(9, E, G.ACTOR)[:3]
    by_id = {i: wide(G.ACTOR, x2, adj2, torch.full((9,), i, dtype=torch.int64)) for i in (0, 63, 64, 127)}
    assert len({bytes(v.cpu().numpy().tobytes()) for v in by_id.values()}) == 4
    for bad, good in ((-5, 0), (128, 127), (1 << 20, 127)):
        assert torch.equal(wide(G.ACTOR, x2, adj2, torch.full((9,), bad, dtype=torch.int64)), by_id[good])
    # types: NaN and negative go to 0, 3.7 truncates to 3, 9 and +inf go to num_embeddings - 1 = 3
    for bad, good in ((float("nan"), 0.0), (-2.0, 0.0), (3.7, 3.0), (9.0, 3.0), (float("inf"), 3.0)):
        xb, xg = x.clone(), x.clone()
        xb[:, 65, -1], xg[:, 65, -1] = bad, good
        xb[:, 3, -1], xg[:, 3, -1] = bad, good
        assert torch.equal(wide(G.ACTOR, xb, adj, ids), wide(G.ACTOR, xg, adj, ids))
    assert bool(torch.isfinite(full).all())


# ---------------------------------------------------------------------------------------------- the table source
NAV = "navigation_graph"
ENGINES = {"nav66": (dict(scenario_name=NAV, num_envs=2, num_agents=33, world_size=6.0, episode_length=4, seed=95, graph_feat_type="global"), 6, 2),
           "nav65": (dict(scenario_name=NAV, num_envs=2, num_agents=30, num_obstacles=5, world_size=6.0, episode_length=4, seed=96,
                          graph_feat_type="global"), 6, 2),
           "nav128": (dict(scenario_name=NAV, num_envs=2, num_agents=64, world_size=12.0, episode_length=4, seed=97, graph_feat_type="global"), 6, 3)}


@functools.lru_cache(maxsize=None)
def recorded(key):
    """(cfg, tables [S, N, W] f64, node_obs [S, N, A, E, F], adj [S, N, E, E]) of S recorded steps of one engine stepped past its time limit, so that
    every env has reset: computed once, never changed"""
    from gmpe.engine import GmpeEngine
    kw, steps, every = ENGINES[key]
    cfg = gmpe.make_config(**kw)
    N, A = cfg.num_envs, cfg.num_agents
    eng = GmpeEngine(cfg, node_form="both", adj_compact=True)
    eng.reset()
    rng = np.random.RandomState(7)
    tabs, rows, adjs = [], [], []
    for t in range(steps):
        o = eng.step(torch.as_tensor(rng.randint(0, cfg.n_actions, (N, A)).astype(np.int32)))
        if t % every == every - 1:
            tabs.append(o.entity_table.clone()); rows.append(o.node_obs.clone()); adjs.append(o.adj.clone())
    eng.check_errors()
    assert steps > cfg.episode_length and cfg.node_feats == 7
    return cfg, torch.stack(tabs).contiguous(), torch.stack(rows).contiguous(), torch.stack(adjs).contiguous()


@pytest.mark.parametrize("which", [G.ACTOR, G.CRITIC])
@pytest.mark.parametrize("key,E,rows", [("nav66", 66, 21), ("nav65", 65, 21), ("nav128", 128, 11)])
def test_the_table_source_gives_the_bits_of_the_engines_own_rows(key, E, rows, which):
    cfg, tabs, node_obs, adj = recorded(key)
    S, N, A, E_, F = node_obs.shape
    assert E_ == E == cfg.num_entities and (E + 31) // 32 == (3 if E < 97 else 4)
    base = device_base(which)
    g = torch.Generator().manual_seed(rows + E)
    idx = torch.randint(0, S * N, (rows,), generator=g)
    idx[1] = idx[0]                                     # a repeat for certain
    ego = torch.randint(0, A, (rows,), generator=g)
    ego[2], ego[3] = A - 1, 0
    idx, ego = idx.to(DEV), ego.to(DEV)
    x = node_obs.reshape(S * N, A, E, F)[idx, ego].contiguous()
    a = adj.reshape(S * N, E, E)[idx].contiguous()
    with torch.no_grad():
        want = gmpe.gnn_base_wide(x, a, ego, base)
        for index in (idx, idx.to(torch.int32)):
            assert torch.equal(gmpe.gnn_base_wide_from_table(tabs, index, ego, base, cfg), want), index.dtype
        # the table_share form: slot s's [N, W] table serves its N * A rows, as the compact adjacency does
        s = S - 1
        egos = torch.arange(A, device=DEV).repeat(N)
        got = gmpe.gnn_base_wide_from_table(tabs[s], None, egos, base, cfg, table_share=A)
        assert torch.equal(got, gmpe.gnn_base_wide(node_obs[s].reshape(N * A, E, F), adj[s], egos, base))
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
    edges = (a > 0) & (a < 1.0)
    assert bool(edges.any()) and not bool(edges.all())


# ---------------------------------------------------------------------------------------------- the C entries
@pytest.mark.parametrize("fill", [0x00, 0xFF])
def test_the_c_entry_on_a_side_stream_writes_features_and_nothing_else(fill):
    n, E, key, _ = case = (9, 128, G.CRITIC, False)
    x, adj, ids = (t.to(DEV) for t in G.inputs(n, E, key)[:3])
    base = device_base(key)
    names, ps, meta = W._base_params(base)
    nbytes, guard = n * G.C * 4, 64
    out = torch.full((guard + nbytes + guard,), fill, dtype=torch.uint8, device=DEV)
    plan = W._plan((n, E, 7, 1, 4, 2), meta, x, adj, ids.to(torch.int32), [p.detach() for p in ps])
    plan.features = out.data_ptr() + guard
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    lib = _lib.load()
    results = []
    for _ in range(2):                                  # a second call gives the same bits
        assert lib.gmpe_gnn_forward_wide(0, C.byref(plan), C.c_void_p(side.cuda_stream)) == 0, lib.gmpe_last_error().decode()
        side.synchronize()
        results.append(out[guard:guard + nbytes].clone().view(torch.float32).view(n, G.C))
        assert bool((out[:guard] == fill).all()) and bool((out[guard + nbytes:] == fill).all())
    assert torch.equal(results[0], results[1]) and torch.equal(results[0], device_run(case))


def test_the_c_table_entry_on_a_side_stream_writes_features_and_nothing_else():
    cfg, tabs, node_obs, adj = recorded("nav66")
    S, N, A, E, F = node_obs.shape
    base = device_base(G.ACTOR)
    names, ps, meta = W._base_params(base)
    rows, guard = N * A, 64
    egos = torch.arange(A, device=DEV, dtype=torch.int32).repeat(N)
    with torch.no_grad():
        want = gmpe.gnn_base_wide(node_obs[0].reshape(rows, E, F), adj[0], egos, base)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    lib = _lib.load()
    for fill in (0x00, 0xFF):
        out = torch.full((guard + rows * G.C * 4 + guard,), fill, dtype=torch.uint8, device=DEV)
        tp = W._table_plan((rows, E, F, 1, 4, 2), meta, cfg, A, tabs[0], None, egos, [p.detach() for p in ps])
        tp.base.features = out.data_ptr() + guard
        torch.cuda.synchronize()
        assert lib.gmpe_gnn_forward_wide_table(0, C.byref(tp), C.c_void_p(side.cuda_stream)) == 0, lib.gmpe_last_error().decode()
        side.synchronize()
        assert torch.equal(out[guard:-guard].clone().view(torch.float32).view(rows, G.C), want)
        assert bool((out[:guard] == fill).all()) and bool((out[-guard:] == fill).all())


# ---------------------------------------------------------------------------------------------- composition at A = 33 (E = 66)
N, A, T, LIMIT = 2, 33, 3, 2
STORED = ("obs", "agent_id", "rewards", "dones", "masks", "active_masks", "value_preds", "available_actions", "actions", "action_log_probs", "rnn_states",
          "rnn_states_critic", "returns")


def setup(**engine_kw):
    from gmpe.engine import GmpeEngine
    from gmpe.rollout import DeviceRolloutBuffer
    from test_gpu_collect import _ValueNorm
    from test_gpu_policy import K, _Net
    from test_gpu_ppo_update import _Critic, update_args
    from test_gpu_parity import ROT
    cfg = gmpe.make_config(scenario_name=ROT, num_envs=N, num_agents=A, world_size=8.0, episode_length=LIMIT, seed=11)
    eng = GmpeEngine(cfg, device=0, **engine_kw)
    assert int(cfg.node_feats) == 7 and int(cfg.n_actions) == K and cfg.num_entities == 66
    actor = _Net(G.ACTOR, eng.D, "act").to(DEV)
    critic = _Critic(G.CRITIC, eng.D, "v_out", seed=12).to(DEV)
    vn = _ValueNorm(DEV)
    vn.running_mean.fill_(0.3), vn.running_mean_sq.fill_(0.7), vn.debiasing_term.fill_(0.5)
    args = update_args(use_popart=False, use_valuenorm=True)
    for k, v in dict(gamma=0.99, gae_lambda=0.95, use_gae=True, use_proper_time_limits=False).items():
        setattr(args, k, v)
    buf = DeviceRolloutBuffer(eng, T, use_centralized_V=False, policy_fields="all", learner_fields="all", args=args, recurrent_N=1, hidden_size=64)
    buf.warmup()
    return cfg, eng, buf, actor, critic, vn, args


def compare(br, bt, what):
    torch.cuda.synchronize()
    for k in STORED:
        x, y = getattr(br, k), getattr(bt, k)
        assert x is not None and y is not None and x.dtype == y.dtype and torch.equal(x, y), (what, k)
    assert float(br.value_preds.abs().max()) > 0 and bool(torch.isfinite(br.returns).all()) and bool(torch.isfinite(br.action_log_probs).all())


def test_collect_steps_and_compute_at_33_agents_on_a_rows_buffer_and_a_table_only_buffer():
    _, er, br, actor, critic, vn, _ = setup()
    cfg, et, bt, _, _, _, _ = setup(node_form="table", adj_form="none")
    assert bt._node_obs is None and bt._adj is None and bt.entity_table is not None and br.entity_table is None
    for b in (br, bt):
        for _ in range(T):
            policy.collect_step(actor, critic, b)
        assert policy.compute(critic, b, copy.deepcopy(vn)) is b.returns and b.step == 0
    compare(br, bt, "collect_step")
    dn = br.dones.bool()
    assert bool(dn.any())                               # the time limit lies inside the window
    assert torch.equal(bt.node_obs, br._node_obs) and torch.equal(bt.adj, br.adj)
    # the stored values are the chain written out on slot 0: gnn_base_wide -> mlp_base -> rnn_layer -> value_head
    with torch.no_grad():
        s = policy._slot_rows(br, 0)
        assert tuple(s["node_obs"].shape) == (N * A, 66, 7)
        nbd = gmpe.gnn_base_wide(s["node_obs"], s["adj"], s["share_agent_id"], critic.gnn_base)
        cent = policy._cent(critic, s["share_obs"])
        f, _ = gmpe.rnn_layer(gmpe.mlp_base(nbd if cent is None else (cent, nbd), critic.base), s["rnn_states_critic"], s["masks"], critic.rnn)
        assert torch.equal(gmpe.value_head(f, critic.v_out).view(N, A, 1), br.value_preds[0])
    # training on this buffer is refused by name
    adv = br.normalized_advantages(vn)
    sample = next(iter(br.feed_forward_generator(adv, 2, perm=torch.randperm(T * N * A, generator=torch.Generator().manual_seed(4)))))
    with pytest.raises(NotImplementedError, match="gnn_base_wide is forward only: backward at E > 64 is not built"):
        policy.minibatch_losses(actor, critic, sample, types.SimpleNamespace())
    for e in (er, et):
        e.check_errors()


@pytest.mark.parametrize("form", ["materialised", "compact", "table"])
def test_evaluator_act_drives_a_batched_evaluator_through_an_episode_at_33_agents(form):
    """either adjacency form an engine hands out; an engine that keeps tables only hands out none, which evaluator_act refuses by name at any E"""
    from gmpe import evaluate as EV
    kw = dict(materialised={}, compact=dict(adj_compact=True), table=dict(node_form="table", adj_form="none"))[form]
    cfg, eng, buf, actor, critic, vn, _ = setup(**kw)
    rnn = torch.zeros((N, A, 1, 64), device=DEV)
    ev = EV.BatchedEvaluator(eng, rnn_states=rnn)
    act = policy.evaluator_act(actor, ev, deterministic=True)
    if form == "table":
        with pytest.raises(ValueError, match="the engine hands out no adjacency"):
            EV.evaluate(eng, act, evaluator=ev)
        return
    got = EV.evaluate(eng, act, evaluator=ev)
    torch.cuda.synchronize()
    assert got["episodes"] == N and bool(torch.isfinite(rnn).all())                # the episode has ended: its envs' states are zeroed again
    eng.check_errors()


def test_one_captured_rollout_replay_is_the_eager_rollout_at_33_agents():
    _, ea, ba, actor, critic, vn, _ = setup()
    _, eb, bb, _, _, _, _ = setup()
    cap = policy.CapturedRollout(actor, critic, bb, vn)
    want, got = policy.rollout(actor, critic, ba, vn), cap.replay()
    assert want is ba.returns and got is bb.returns
    compare(ba, bb, "captured rollout")
    for e in (ea, eb):
        e.check_errors()
