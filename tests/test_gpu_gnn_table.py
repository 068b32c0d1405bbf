"""The policy's GNNBase straight from the entity table (gmpe.gnn_base_from_table, gmpe_gnn_forward_table / gmpe_gnn_backward_table) against gmpe.gnn_base on
the rows and the adjacency the SAME engine wrote next to that table (node_form="both", adj_compact=True): the features and every parameter gradient, bit for
bit, for equal `rows`. No tolerance anywhere. The tables come from real engines stepped with random actions through goal reaches (masked rows and columns,
the ordered-visibility rule) and auto-resets; all three row kinds and the `two` flag; E = 6, 20 and 44 (two mask words).

The two-mask-word case: the issue names the 32-agent + 8-obstacle + 4-wall config as "E = 44", but that config has 32 + 32 + 8 = 72 entities, more than the 64
nodes the GNN kernels are built for (tests/test_gnn_table_host.py pins that refusal). The case here keeps E = 44, the 8 obstacles, the 4 walls and N = 2, with
18 agents."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import gmpe
import gnn_lib as G
import oracle_lib as ol
from gmpe import _lib
from test_gpu_gather import JULY, _queue
from test_gpu_parity import ROT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAV = "navigation_graph"
# key -> (config keywords, steps, record every)
ENGINES = {
    "july": (dict(scenario_name=JULY, num_envs=16, num_agents=3, world_size=2.4, episode_length=30, seed=91), 60, 5),
    "rot_inv": (dict(scenario_name=ROT, num_envs=16, num_agents=3, world_size=2.4, episode_length=30, seed=92), 60, 5),
    "two_phase": (dict(scenario_name="two_phase_graph", num_envs=16, num_agents=3, world_size=2.4, episode_length=30, seed=93), 60, 5),
    "global": (dict(scenario_name=JULY, num_envs=16, num_agents=3, world_size=2.4, episode_length=30, seed=94, graph_feat_type="global"), 60, 5),
    "nav20": (dict(scenario_name=NAV, num_envs=8, num_agents=7, num_obstacles=6, world_size=2.4, episode_length=8, seed=95), 20, 4),
    "nav44": (dict(scenario_name=NAV, num_envs=2, num_agents=18, num_obstacles=8, num_walls=4, world_size=4.0, episode_length=6, seed=96), 14, 2),
}
SMALL = ("july", "rot_inv", "two_phase", "global")      # E = 6
KINDS = {"july": (0, 0, 8), "rot_inv": (1, 0, 7), "two_phase": (1, 1, 7), "global": (2, 0, 7), "nav20": (0, 0, 8), "nav44": (0, 0, 8)}


@functools.lru_cache(maxsize=None)
def recorded(key):
    """(cfg, tables [S, N, W] f64, node_obs [S, N, A, E, F], adj [S, N, E, E]) of S recorded steps of one engine: computed once, never changed"""
    from gmpe.engine import GmpeEngine
    kw, steps, every = ENGINES[key]
    cfg = gmpe.make_config(**kw)
    N, A = cfg.num_envs, cfg.num_agents
    nav = kw["scenario_name"] == NAV
    eng = GmpeEngine(cfg, node_form="both", adj_compact=True)
    o = eng.reset()
    rng = np.random.RandomState(7)
    if not nav:                                         # queued in front of the tube: goal reaches and heading re-draws within ~30 steps
        orc = ol.Oracle(cfg)
        orc.reset()
        _queue(orc, (eng,), rng, N, A)
    tabs, rows, adjs, done_seen = [], [], [], 0
    for t in range(steps):
        act = (rng.randint(0, cfg.n_actions, (N, A)) if nav else np.where(rng.rand(N, A) < 0.7, 14, rng.randint(0, 25, (N, A)))).astype(np.int32)
        o = eng.step(torch.as_tensor(act))
        done_seen += int(eng.get("status").astype(bool).sum())
        if t % every == every - 1:
            tabs.append(o.entity_table.clone()); rows.append(o.node_obs.clone()); adjs.append(o.adj.clone())
    eng.check_errors()
    assert steps > cfg.episode_length                   # some envs have reset
    tabs = torch.stack(tabs)
    if not nav:
        assert done_seen > 0 and bool((tabs[..., -1] != 0).any())      # some agents are done: their mask bits are set in a recorded table
    kind, two, F = KINDS[key]
    assert cfg.node_feats == F and tabs.shape[-1] == cfg.entity_table_width
    return cfg, tabs.contiguous(), torch.stack(rows).contiguous(), torch.stack(adjs).contiguous()


@functools.lru_cache(maxsize=None)
def module(F, which):
    """the shipped actor ('node') or critic (global mean) GNNBase for F node features, from tests/golden/gnn_base.npz"""
    if F == 7:
        cfg = G.config("actor") if which == "actor" else G.config("critic")
    else:
        cfg = G.config("rotate") if which == "actor" else G.config("rotate", aggr="mean")
    return G.build(cfg).to(DEV)


def grads_of(f, base, gf):
    ps = list(base.parameters())
    return [f.detach()] + list(torch.autograd.grad((f * gf).sum(), ps))


def draw(key, rows, seed, dtype=torch.int64):
    """a permuted index with repeats over all recorded slots, the egos, the output gradient"""
    cfg, tabs, _, _ = recorded(key)
    S, N, _ = tabs.shape
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, S * N, (rows,), generator=g)
    if rows >= 5:
        idx[1] = idx[0]                                 # a repeat for certain
    ego = torch.randint(0, cfg.num_agents, (rows,), generator=g)
    gf = torch.randn((rows, G.C), generator=g)
    return idx.to(dtype).to(DEV), ego.to(DEV), gf.to(DEV)


def both(key, which, idx, ego, gf):
    """[features, grads...] of gnn_base_from_table and of gnn_base on the engine's own arrays"""
    cfg, tabs, node_obs, adj = recorded(key)
    S, N, A, E, F = node_obs.shape
    base = module(F, which)
    got = grads_of(gmpe.gnn_base_from_table(tabs, idx, ego, base, cfg), base, gf)
    li = idx.long()
    x = node_obs.reshape(S * N, A, E, F)[li, ego.long()].contiguous()
    a = adj.reshape(S * N, E, E)[li].contiguous()
    want = grads_of(gmpe.gnn_base(x, a, ego, base), base, gf)
    return got, want


def assert_equal(got, want, what):
    names = ["features"] + ["grad %d" % i for i in range(len(got) - 1)]
    for n, a, b in zip(names, got, want):
        assert a.shape == b.shape and torch.equal(a, b), "%s: %s differs" % (what, n)
    assert bool(torch.isfinite(got[0]).all()) and float(got[0].abs().max()) > 0


@pytest.mark.parametrize("which", ["actor", "critic"])
@pytest.mark.parametrize("rows", [1, 5, 65, 1025])      # 1025: the smallest count at which one of the 256 workgroups owns a second tile of four
@pytest.mark.parametrize("key", SMALL)
def test_forward_and_every_gradient_are_gnn_bases_bits_on_the_engines_own_rows(key, rows, which):
    idx, ego, gf = draw(key, rows, 100 + rows)
    got, want = both(key, which, idx, ego, gf)
    assert_equal(got, want, "%s %s rows=%d" % (key, which, rows))
    if rows == 65:                                      # the int32 index: the same bits
        got32, _ = both(key, which, idx.to(torch.int32), ego, gf)
        assert_equal(got32, want, "%s %s int32 index" % (key, which))


@pytest.mark.parametrize("which", ["actor", "critic"])
@pytest.mark.parametrize("key,rows", [("nav20", 33), ("nav44", 12)])
def test_obstacles_and_two_mask_words(key, rows, which):
    cfg = recorded(key)[0]
    assert cfg.num_entities == (20 if key == "nav20" else 44) and (cfg.num_entities + 31) // 32 == (1 if key == "nav20" else 2)
    idx, ego, gf = draw(key, rows, 7)
    got, want = both(key, which, idx, ego, gf)
    assert_equal(got, want, "%s %s" % (key, which))


@pytest.mark.parametrize("key", SMALL + ("nav20",))
def test_the_table_share_form_is_a_rollout_steps_rows(key):
    """table_index None, table_share = A: slot s's [N, W] table serves its N * A rows, as gnn_base's compact adjacency does; under no_grad too"""
    cfg, tabs, node_obs, adj = recorded(key)
    S, N, A, E, F = node_obs.shape
    s = S - 1
    ego = torch.arange(A, device=DEV).repeat(N)
    gf = torch.randn((N * A, G.C), generator=torch.Generator().manual_seed(3)).to(DEV)
    for which in ("actor", "critic"):
        base = module(F, which)
        got = grads_of(gmpe.gnn_base_from_table(tabs[s], None, ego, base, cfg, table_share=A), base, gf)
        want = grads_of(gmpe.gnn_base(node_obs[s].reshape(N * A, E, F), adj[s], ego, base), base, gf)
        assert_equal(got, want, "%s %s share" % (key, which))
        with torch.no_grad():
            f = gmpe.gnn_base_from_table(tabs[s], None, ego.view(-1, 1).float(), base, cfg, table_share=A)
        assert not f.requires_grad and torch.equal(f, want[0])


def test_clamped_indices_and_egos_run_clean():
    """an index outside the table and an ego outside [0, A) are clamped: nothing is read out of bounds, the other rows keep their bits, and the run ends clean"""
    key = "rot_inv"
    cfg, tabs, node_obs, adj = recorded(key)
    S, N = tabs.shape[:2]
    idx, ego, gf = draw(key, 65, 11)
    base = module(cfg.node_feats, "actor")
    clean = gmpe.gnn_base_from_table(tabs, idx, ego, base, cfg).detach()
    bad_i, bad_e = idx.clone(), ego.clone()
    bad_i[3], bad_i[9], bad_e[20], bad_e[31] = -5, 1 << 40, -3, 99
    f = gmpe.gnn_base_from_table(tabs, bad_i, bad_e, base, cfg)
    (f * gf).sum().backward()
    torch.cuda.synchronize()
    keep = torch.ones(65, dtype=torch.bool, device=DEV)
    keep[[3, 9, 20, 31]] = False
    assert torch.equal(f.detach()[keep], clean[keep]) and bool(torch.isfinite(f).all())
    # a clamped index reads the table's first or last row; what a clamped ego's row holds is unspecified (the view and the 'node' gather clamp on their own)
    fix_i = idx.clone()
    fix_i[3], fix_i[9] = 0, S * N - 1
    keep[[3, 9]] = True
    assert torch.equal(f.detach()[keep], gmpe.gnn_base_from_table(tabs, fix_i, ego, base, cfg).detach()[keep])
    for p in base.parameters():
        assert bool(torch.isfinite(p.grad).all())
        p.grad = None
    bad32 = bad_i.clamp(-5, 2 ** 31 - 1).to(torch.int32)
    assert torch.equal(gmpe.gnn_base_from_table(tabs, bad32, bad_e, base, cfg).detach(), f.detach())


# ---------------------------------------------------------------------------------------------- the C entries
GUARD = 3
PAD = 64                                                # guard bytes on both sides of the workspace


def c_call(key, which, idx, ego, gf, stream=None, share=None):
    """gmpe_gnn_forward_table (+ gmpe_gnn_backward_table, twice) through ctypes with caller-owned buffers -> [features, grads...]"""
    from gmpe import gnn as W
    lib = _lib.load()
    cfg, tabs, _, _ = recorded(key)
    base = module(cfg.node_feats, which)
    names, ps, meta = W._base_params(base)
    ps = [p.detach().contiguous() for p in ps]
    rows = int(ego.shape[0])
    shape = (rows, cfg.num_entities, cfg.node_feats, 1, int(ps[0].shape[0]), int(ps[0].shape[1]))
    table = tabs if share is None else tabs[-1]
    ids = ego.to(torch.int32)                           # the plan holds addresses: every array it names lives to the end of this function
    tp = W._table_plan(shape, meta, cfg, share or 0, table, idx, ids, ps)
    nan = float("nan")
    f = torch.full((rows + GUARD, G.C), nan, device=DEV)
    tp.base.features = f.data_ptr()
    st = C.c_void_p((stream or torch.cuda.current_stream(torch.device(DEV))).cuda_stream)
    _lib.check(lib.gmpe_gnn_forward_table(0, C.byref(tp), st), "gmpe_gnn_forward_table")
    nbytes = C.c_size_t()
    _lib.check(lib.gmpe_gnn_workspace_bytes(C.byref(tp.base), 1, C.byref(nbytes)), "gmpe_gnn_workspace_bytes")
    nbytes = nbytes.value
    assert nbytes % 8 == 0 and nbytes == gmpe.gnn_workspace_bytes(rows, shape[1], shape[2], meta[0], meta[1], meta[2], shape[4], shape[5])
    ws = torch.full((PAD + nbytes + PAD,), 0xA5, dtype=torch.uint8, device=DEV)
    gps = [torch.full((t.numel() + GUARD,), nan, device=DEV) for t in ps]
    tp.base.workspace, tp.base.workspace_bytes, tp.base.grad_features, tp.base.features = ws.data_ptr() + PAD, nbytes, gf.data_ptr(), None
    W._fill(tp.base, meta, meta[5], meta[2], meta[1], gps, "grad_")
    first = None
    for rep in range(2):                                # backward may be repeated on one plan: the same bits
        _lib.check(lib.gmpe_gnn_backward_table(0, C.byref(tp), st), "gmpe_gnn_backward_table")
        if rep == 0:
            torch.cuda.synchronize()
            first = [g.clone() for g in gps]
            for g in gps:
                g.fill_(nan)
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    assert bool((ws[:PAD] == 0xA5).all()) and bool((ws[PAD + nbytes:] == 0xA5).all()), "bytes around the workspace were written"
    assert bool(torch.isnan(f[rows:]).all()), "rows past the end of features were written"
    out = [f[:rows].clone()]
    by_id = {id(p): i for i, p in enumerate(base.parameters())}
    grads = [None] * len(by_id)
    for like, g, g1 in zip(W._base_params(base)[1], gps, first):
        assert torch.equal(g[:like.numel()], g1[:like.numel()]), "the second backward call differs"
        assert bool(torch.isnan(g[like.numel():]).all()), "elements past the end of a gradient were written"
        grads[by_id[id(like)]] = g[:like.numel()].reshape(like.shape).clone()
    return out + grads


@pytest.mark.parametrize("key,which", [("july", "actor"), ("two_phase", "critic"), ("nav44", "actor")])
def test_the_c_entries_give_the_wrappers_bits_stay_inside_their_buffers_and_run_on_a_side_stream(key, which):
    rows = 65 if key != "nav44" else 12
    idx, ego, gf = draw(key, rows, 21)
    _, want = both(key, which, idx, ego, gf)
    assert_equal(c_call(key, which, idx, ego, gf), want, "C entries " + key)
    assert_equal(c_call(key, which, idx.to(torch.int32), ego, gf), want, "C entries int32 " + key)
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        other = c_call(key, which, idx, ego, gf, stream=side)
    assert_equal(other, want, "C entries on a side stream " + key)
