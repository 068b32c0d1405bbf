"""The fp64 entity table (include/gmpe.h gmpe_outputs.entity_table) restated in NumPy: the truth of every kernel that rebuilds node rows and adjacency
entries from it with csrc/gmpe_expand.h — k_node_expand / k_adj_from_table, k_mb_table, the GMPE_MBE_TABLE source of gmpe_minibatch_edges and the table
source of the narrow and wide GNN kernels.

rows_and_adj repeats node_row_from_table<KIND> and adj_entry_from_table operation for operation. Every operation there is one IEEE add, sub, mul, sqrt or
cast (the header's users are compiled with -ffp-contract=off), and NumPy's are the same correctly rounded operations, so the kernels are compared with it
by array_equal, without a tolerance. tests/test_table_host.py holds it to the oracle's step outputs; synthetic() makes hand-made tables whose mask words have
bits where no engine run of the suite puts them."""
import numpy as np

from gmpe.config import ROT_FAMILY, SCENARIO_TWO_PHASE

NAV, ROT, TWO = "navigation_graph", "nav_graph_metered_single_corridor_rot_inv", "two_phase_graph"
# kind of node row -> make_config keywords: 0 relative (F = 8), 1 rot_inv family (F = 7), "two" = 1 with the corridor exit as every goal, 2 global (F = 7)
KINDS = {0: dict(scenario_name=NAV), 1: dict(scenario_name=ROT), "two": dict(scenario_name=TWO), 2: dict(scenario_name=NAV, graph_feat_type="global")}
# E -> (agents, landmarks, obstacles): 33 the first bit of word 1 and E * E % 4 != 0; 64 two full words; 65 the scalar path and a word with one valid bit;
# 66; 97 and 128 four words, the wide GNN kernel's second wave
SHAPES = {33: (16, 16, 1), 64: (32, 32, 0), 65: (30, 30, 5), 66: (33, 33, 0), 97: (48, 48, 1), 128: (64, 64, 0)}
# side of the world of a synthetic table: about ten neighbours within max_edge_dist = 1 of a node
SIDE = {33: 3.2, 64: 4.5, 65: 4.5, 66: 4.5, 97: 5.5, 128: 6.3}


def config(E, kind, num_envs=2, **kw):
    import gmpe
    A, L, O = SHAPES[E]
    c = dict(KINDS[kind], num_envs=num_envs, num_agents=A, num_landmarks=L, num_obstacles=O, world_size=SIDE[E])
    c.update(kw)
    return gmpe.make_config(**c)


def row_kind(cfg):
    """(KIND, two) as gmpe_expand_node_obs picks its kernel"""
    kind = 2 if cfg.graph_feat_type == 1 else (1 if cfg.scenario in ROT_FAMILY else 0)
    return kind, int(cfg.scenario == SCENARIO_TWO_PHASE)


def layout(cfg):
    """offsets, in doubles, of the columns of one table row (config.entity_table_width): x[E], y[E], vox / voy / vnx / vny [A], cos / sin [A] (rot_inv
    family), the exit x, y (two_phase), ceil(E / 32) mask words; absent columns are None"""
    A, E = cfg.num_agents, cfg.num_entities
    words = (E + 31) // 32
    rot, two = cfg.scenario in ROT_FAMILY, cfg.scenario == SCENARIO_TWO_PHASE
    o = dict(x=0, y=E, vox=2 * E, voy=2 * E + A, vnx=2 * E + 2 * A, vny=2 * E + 3 * A, cos=None, sin=None, exit=None)
    cur = 2 * E + 4 * A
    if rot:
        o["cos"], o["sin"], cur = cur, cur + A, cur + 2 * A
    if two:
        o["exit"], cur = cur, cur + 2
    o["mask"], o["words"], o["width"] = cur, words, cur + words
    assert o["width"] == cfg.entity_table_width
    return o


def mask_bits(cfg, table):
    """[.., E] bool from the mask words: bit k & 31 of (unsigned)word[k >> 5]"""
    lay = layout(cfg)
    E = cfg.num_entities
    w = np.asarray(table)[..., lay["mask"]:lay["width"]].astype(np.uint64).astype(np.uint32)
    k = np.arange(E)
    return ((w[..., k >> 5] >> (k & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)


def rows_and_adj(cfg, table):
    """table [.., W] f64 -> (node_obs [.., A, E, F] f32, adj [.., E, E] f32, masked [.., E] bool): gmpe_expand.h in NumPy"""
    table = np.asarray(table, dtype=np.float64)
    lead = table.shape[:-1]
    T = table.reshape(-1, table.shape[-1])
    B = T.shape[0]
    lay = layout(cfg)
    A, L, E = cfg.num_agents, cfg.num_landmarks, cfg.num_entities
    kind, two = row_kind(cfg)
    f32, f64 = np.float32, np.float64
    ex, ey = T[:, :E], T[:, E:2 * E]
    kag = np.arange(E) < A
    post = (np.arange(E)[None, :] <= np.arange(A)[:, None])[None]            # [1, A, E]: agent k's re-drawn velocity is visible to ego ei iff k <= ei
    typ = np.where(kag, 0.0, np.where(np.arange(E) < A + L, 1.0, 2.0)).astype(f32)

    def per_entity(off, dtype):                                              # an agent column as [B, E]: 0 for the other entities
        out = np.zeros((B, E), dtype=dtype)
        out[:, :A] = T[:, off:off + A].astype(dtype)
        return out

    def goal(pos, other):                                                    # agent k: its landmark A + k; another entity: `other`
        out = np.array(other, dtype=pos.dtype, copy=True)
        out[:, :A] = pos[:, A:2 * A]
        return out

    F = 8 if kind == 0 else 7
    rows = np.zeros((B, A, E, F), dtype=f32)
    if kind == 0:
        kvox, kvoy, kvnx, kvny = (per_entity(lay[n], f64) for n in ("vox", "voy", "vnx", "vny"))
        gx, gy = goal(ex, ex), goal(ey, ey)
        px, py = ex[:, :A, None], ey[:, :A, None]
        evx, evy = T[:, lay["vnx"]:lay["vnx"] + A, None], T[:, lay["vny"]:lay["vny"] + A, None]
        rows[..., 0] = (np.where(post, kvnx[:, None], kvox[:, None]) - evx).astype(f32)
        rows[..., 1] = (np.where(post, kvny[:, None], kvoy[:, None]) - evy).astype(f32)
        rows[..., 2] = (ex[:, None] - px).astype(f32)
        rows[..., 3] = (ey[:, None] - py).astype(f32)
        rows[..., 4] = (gx[:, None] - px).astype(f32)
        rows[..., 5] = (gy[:, None] - py).astype(f32)
        rows[..., 6] = np.where(kag, f32(0), f32(1))
        rows[..., 7] = typ
    elif kind == 1:
        kx, ky = ex.astype(f32), ey.astype(f32)
        kvox, kvoy, kvnx, kvny = (per_entity(lay[n], f32) for n in ("vox", "voy", "vnx", "vny"))
        if two:                                                              # exit x, y right before the mask words
            gxk = np.broadcast_to(T[:, lay["mask"] - 2].astype(f32)[:, None], (B, E))
            gyk = np.broadcast_to(T[:, lay["mask"] - 1].astype(f32)[:, None], (B, E))
        else:
            gxk, gyk = goal(kx, np.zeros((B, E), f32)), goal(ky, np.zeros((B, E), f32))
        apx, apy = kx[:, :A, None], ky[:, :A, None]
        avx, avy = T[:, lay["vnx"]:lay["vnx"] + A].astype(f32)[:, :, None], T[:, lay["vny"]:lay["vny"] + A].astype(f32)[:, :, None]
        cs, sn = T[:, lay["cos"]:lay["cos"] + A, None], T[:, lay["sin"]:lay["sin"] + A, None]
        rvx, rvy = np.where(post, kvnx[:, None], kvox[:, None]) - avx, np.where(post, kvny[:, None], kvoy[:, None]) - avy
        rpx, rpy = kx[:, None] - apx, ky[:, None] - apy
        gdx, gdy = gxk[:, None] - apx, gyk[:, None] - apy
        assert rvx.dtype == rpx.dtype == gdx.dtype == f32                    # the differences are float32 operations

        def rot2(vx, vy):                                                    # two products and a sum, in double
            vx, vy = vx.astype(f64), vy.astype(f64)
            return cs * vx + sn * vy, (-sn) * vx + cs * vy

        o0, o1 = rot2(rvx, rvy)
        o2, o3 = rot2(rpx, rpy)
        o4, o5 = rot2(gdx, gdy)
        o4, o5 = np.where(kag, o4, o2), np.where(kag, o5, o3)
        for i, o in enumerate((o0, o1, o2, o3, o4, o5)):
            rows[..., i] = o.astype(f32)
        rows[..., 6] = typ
    else:
        kx, ky = ex.astype(f32), ey.astype(f32)
        kvox, kvoy, kvnx, kvny = (per_entity(lay[n], f32) for n in ("vox", "voy", "vnx", "vny"))
        rows[..., 0] = np.where(post, kvnx[:, None], kvox[:, None])
        rows[..., 1] = np.where(post, kvny[:, None], kvoy[:, None])
        rows[..., 2], rows[..., 3] = kx[:, None], ky[:, None]
        rows[..., 4], rows[..., 5] = goal(kx, kx)[:, None], goal(ky, ky)[:, None]
        rows[..., 6] = typ
    # the adjacency: delta = pos[min(r, c)] - pos[max(r, c)], f32(sqrt(dx * dx + dy * dy)), zero diagonal, masked rows and columns zero
    r, c = np.arange(E)[:, None], np.arange(E)[None, :]
    lo, hi = np.minimum(r, c), np.maximum(r, c)
    dx, dy = ex[:, lo] - ex[:, hi], ey[:, lo] - ey[:, hi]
    masked = mask_bits(cfg, T)
    zero = (r == c)[None] | masked[:, :, None] | masked[:, None, :]
    adj = np.where(zero, f32(0), np.sqrt(dx * dx + dy * dy).astype(f32))
    assert rows.dtype == f32 and adj.dtype == f32
    return rows.reshape(lead + (A, E, F)), adj.reshape(lead + (E, E)), masked.reshape(lead + (E,))


def force_done(target, agents):
    """agents (not all of an env: that would reset it) done, each on its own landmark: status = 1 and goal_tracker = i through .get / .set, on a GmpeEngine
    or an oracle_lib.Oracle. The next step masks node i and node A + i."""
    agents = np.asarray(agents)
    st, gt = target.get("status"), target.get("goal_tracker")
    assert 0 < len(agents) < st.shape[1]
    st[:, agents] = 1
    gt[:, agents] = agents
    target.set("status", st)
    target.set("goal_tracker", gt)


def implied_mask(cfg, agents):
    """[E] bool: what force_done(agents) makes the next step's mask words say"""
    m = np.zeros(cfg.num_entities, dtype=bool)
    m[np.asarray(agents)] = True
    m[cfg.num_agents + np.asarray(agents)] = True
    return m


def words_of(masked):
    """[.., E] bool -> [.., ceil(E / 32)] uint32: bit k & 31 of word k >> 5; no bit at or above E"""
    masked = np.asarray(masked, dtype=bool)
    E = masked.shape[-1]
    words = (E + 31) // 32
    pad = np.zeros(masked.shape[:-1] + (words * 32,), dtype=np.uint64)
    pad[..., :E] = masked
    return (pad.reshape(masked.shape[:-1] + (words, 32)) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


PATTERNS = ("none", "node 0", "bit 31 of every word", "node E - 1", "node 32", "node 64", "a random half", "everything")


def pattern(name, E, rng):
    m = np.zeros(E, dtype=bool)
    if name == "node 0":
        m[0] = True
    elif name == "bit 31 of every word":
        m[31::32] = True
    elif name == "node E - 1":
        m[E - 1] = True
    elif name == "node 32":
        m[32] = True
    elif name == "node 64":
        m[64] = True
    elif name == "a random half":
        m[rng.permutation(E)[:E // 2]] = True
    elif name == "everything":
        m[:] = True
    else:
        assert name == "none"
    return m


def patterns(E, seed=0):
    """the required mask patterns that exist at E, as (names, [n, E] bool)"""
    rng = np.random.RandomState(5000 + E + seed)
    names = [n for n in PATTERNS if (n != "node 64" or E > 64) and (n != "node 32" or E > 32)]
    return names, np.stack([pattern(n, E, rng) for n in names])


def synthetic(cfg, n, seed, masked):
    """n hand-made tables [n, W]: positions uniform in the world, velocities N(0, 1) with vn != vo for every second agent (so that the ordered-visibility
    rule shows), cos / sin of a drawn heading, a drawn exit, and the mask words of masked [n, E] as float64(uint32)"""
    lay = layout(cfg)
    A, E = cfg.num_agents, cfg.num_entities
    masked = np.asarray(masked, dtype=bool)
    assert masked.shape == (n, E)
    rng = np.random.RandomState(seed)
    half = cfg.world_size / 2.0
    T = np.zeros((n, lay["width"]), dtype=np.float64)
    T[:, :2 * E] = rng.uniform(-half, half, (n, 2 * E))
    vo, vn = rng.randn(n, 2 * A), rng.randn(n, 2 * A)
    same = np.tile(np.arange(A) % 2 == 0, 2)
    vn[:, same] = vo[:, same]
    T[:, lay["vox"]:lay["vox"] + 2 * A], T[:, lay["vnx"]:lay["vnx"] + 2 * A] = vo, vn
    if lay["cos"] is not None:
        th = rng.uniform(-np.pi, np.pi, (n, A))
        T[:, lay["cos"]:lay["cos"] + A], T[:, lay["sin"]:lay["sin"] + A] = np.cos(th), np.sin(th)
    if lay["exit"] is not None:
        T[:, lay["exit"]:lay["exit"] + 2] = rng.uniform(-half, half, (n, 2))
    T[:, lay["mask"]:] = words_of(masked).astype(np.float64)
    return T


def synthetic_patterns(cfg, seed, repeat=1):
    """one table per required pattern (repeat > 1: that many draws of each) -> (names, tables [n, W], masked [n, E])"""
    names, m = patterns(cfg.num_entities, seed)
    names, m = names * repeat, np.tile(m, (repeat, 1))
    return names, synthetic(cfg, len(names), seed, m), m


# ---------------------------------------------------------------------------------------------- graphs for the GNN kernels
# (E, kind, gnn_lib configuration) -> the seed of the case's synthetic tables: the first one at which every graph of the case keeps gnn_lib.MARGIN in
# front of every ReLU of the float64 truth (tests/test_table_host.py checks each on the CPU), so that no graph is dropped from a comparison
GNN_WEIGHTS = ((0, "ROTATE"), (1, "ACTOR"), (1, "CRITIC"), ("two", "ACTOR"), ("two", "CRITIC"), (2, "ACTOR"))
GNN_SEEDS = {(33, 0, "ROTATE"): 33001, (33, 1, "ACTOR"): 33000, (33, 1, "CRITIC"): 33000, (33, "two", "ACTOR"): 33001, (33, "two", "CRITIC"): 33000,
             (33, 2, "ACTOR"): 33000, (64, 0, "ROTATE"): 64000, (64, 1, "ACTOR"): 64001, (64, 1, "CRITIC"): 64001, (64, "two", "ACTOR"): 64004,
             (64, "two", "CRITIC"): 64009, (64, 2, "ACTOR"): 64000, (65, 0, "ROTATE"): 65000, (65, 1, "ACTOR"): 65000, (65, 1, "CRITIC"): 65000,
             (65, "two", "ACTOR"): 65000, (65, "two", "CRITIC"): 65000, (65, 2, "ACTOR"): 65000, (66, 0, "ROTATE"): 66001, (66, 1, "ACTOR"): 66000,
             (66, 1, "CRITIC"): 66000, (66, "two", "ACTOR"): 66003, (66, "two", "CRITIC"): 66000, (66, 2, "ACTOR"): 66002, (97, 0, "ROTATE"): 97001,
             (97, 1, "ACTOR"): 97000, (97, 1, "CRITIC"): 97002, (97, "two", "ACTOR"): 97003, (97, "two", "CRITIC"): 97004, (97, 2, "ACTOR"): 97001,
             (128, 0, "ROTATE"): 128001, (128, 1, "ACTOR"): 128000, (128, 1, "CRITIC"): 128000, (128, "two", "ACTOR"): 128000,
             (128, "two", "CRITIC"): 128000, (128, 2, "ACTOR"): 128000}


def gnn_case(E, kind, weights, seed=None):
    """One table per required mask pattern and 2 n + 1 graphs over them, every table twice and a repeat: -> dict(cfg, names, tables [n, W], idx, ego,
    x [rows, E, F], adj [rows, E, E] (the restated rows and adjacency of each graph), key (the gnn_lib configuration))"""
    import gnn_lib as G
    seed = GNN_SEEDS[(E, kind, weights)] if seed is None else seed
    cfg = config(E, kind)
    names, tables, _ = synthetic_patterns(cfg, seed)
    n, A = len(names), cfg.num_agents
    rng = np.random.RandomState(seed + 1)
    idx = np.concatenate([np.arange(n), np.arange(n), [0]]).astype(np.int64)
    ego = rng.randint(0, A, len(idx)).astype(np.int64)
    ego[0], ego[1], ego[-1] = 0, A - 1, 0                                    # the first and the last agent; graph 2 n repeats graph 0
    rows, adj, _ = rows_and_adj(cfg, tables)
    return dict(cfg=cfg, names=names, tables=tables, idx=idx, ego=ego, x=np.ascontiguousarray(rows[idx, ego]), adj=np.ascontiguousarray(adj[idx]),
                key=getattr(G, weights))


def gnn_margins(case):
    """per graph, the smallest |pre-activation| in front of a ReLU of the float64 truth"""
    import gnn_lib as G
    import torch
    base64 = G.build(G.CONFIGS[case["key"]], torch.float64)
    return G.margins(base64, torch.from_numpy(case["x"]), torch.from_numpy(case["adj"]), torch.from_numpy(case["ego"])).numpy()


def gnn_truth(case):
    """-> (features of the float64 restatement of tests/gnn_lib.py [rows, 16], err_ref of the same restatement in float32 on the CPU)"""
    import gnn_lib as G
    import torch
    x, adj, ids = torch.from_numpy(case["x"]), torch.from_numpy(case["adj"]), torch.from_numpy(case["ego"])
    with torch.no_grad():
        t = G.forward(G.build(G.CONFIGS[case["key"]], torch.float64), x.double(), adj.double(), ids).numpy()
        r = G.forward(G.build(G.CONFIGS[case["key"]], torch.float32), x, adj, ids).double().numpy()
    return t, G.err(r, t)
