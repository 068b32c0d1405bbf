"""gmpe_minibatch_gather driven through its C entry (ctypes on gmpe._lib.GmpeMinibatchPlan), where gmpe.minibatch.Gather never goes: src / dst 4, 8 and 12 bytes
past a 256-byte boundary, slot strides wider than one slot, out-of-range permutation entries, MAX_FIELDS fields and fields of 255 / 256 / 257 threads, cfg = NULL,
the recurrent map at L = 1, L = T, L > T, A = 1, N = 1 and one chunk, the table kinds to misaligned and strided outputs, two calls, and a captured graph.

Each test owns one device uint8 buffer: destinations with at least 256 sentinel bytes around each, then the sources. After the call the whole buffer is compared
with the image tests/minibatch_lib.py gather_bytes makes of the header's sentences (tests/test_minibatch_host.py pins it to the reference's yields and shows
which case of KERNEL_CASES tells which mistake), so copied rows, unwritten rows, gaps and guards are checked at once. The table kinds' rows are the rows-form
engine's own node_obs and adj of the same rollout. Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import gmpe
from gmpe import _lib
import minibatch_lib as M
from test_gpu_gather import JULY, _queue

pytestmark = pytest.mark.gpu
ROT_INV = "nav_graph_metered_single_corridor_rot_inv"
CASES = {c["name"]: c for c in M.KERNEL_CASES}


def _c_plan(plan, base, perm):
    p = _lib.GmpeMinibatchPlan()
    p.mode, p.num_fields, p.T, p.N, p.A, p.L = plan["mode"], len(plan["fields"]), plan["T"], plan["N"], plan["A"], plan["L"]
    p.perm, p.perm_len, p.offset, p.rows = perm.data_ptr(), int(perm.shape[0]), plan["offset"], plan["rows"]
    for c, f in zip(p.fields, plan["fields"]):
        c.kind, c.row_bytes, c.slot_stride, c.src, c.dst = f["kind"], f["row_bytes"], f["slot_stride"], base + f["src"], base + f["dst"]
    return p


def _upload(torch, plan, image):
    buf, perm = torch.from_numpy(image).cuda(), torch.from_numpy(plan["perm"]).cuda()
    assert buf.data_ptr() % 256 == 0 and perm.data_ptr() % 8 == 0 and buf.dtype == torch.uint8 and perm.dtype == torch.int64
    return buf, perm


def _launch(torch, plan, buf, perm, cfg=None):
    """one gmpe_minibatch_gather on the current stream; cfg None: the NULL config"""
    rc = _lib.load().gmpe_minibatch_gather(None if cfg is None else C.byref(cfg), 0, C.byref(_c_plan(plan, buf.data_ptr(), perm)),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "gmpe_minibatch_gather")


def _gather(torch, plan, image, cfg=None):
    buf, perm = _upload(torch, plan, image)
    _launch(torch, plan, buf, perm, cfg)
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def _same_image(got, want, plan, what):
    """the whole buffer, byte for byte; on a difference, say in which field's output (or outside all of them) it lies"""
    if np.array_equal(got, want):
        return
    bad = np.flatnonzero(got != want)
    inside, where = np.zeros(bad.size, dtype=bool), []
    for i, f in enumerate(plan["fields"]):
        lo, rb = f["dst"], f["row_bytes"]
        hit = (bad >= lo) & (bad < lo + M.out_rows(plan, f["kind"]) * rb)
        inside |= hit
        if hit.any():
            where.append("field %d (kind %d, %d-byte rows, stride %d, src %% 16 = %d, dst %% 16 = %d): %d bytes, first in row %d"
                         % (i, f["kind"], rb, f["slot_stride"], f["src"] % 16, f["dst"] % 16, int(hit.sum()), (int(bad[hit][0]) - lo) // rb))
    raise AssertionError("%s: %d bytes differ, %d outside every output (first at %d); %s" % (what, bad.size, int((~inside).sum()), int(bad[0]), "; ".join(where)))


@pytest.mark.parametrize("name", [c["name"] for c in M.KERNEL_CASES])
def test_copy_kinds_equal_the_byte_level_restatement(name):
    """alignments and strides (align_*, widths_alone), the work list (wl_*, single), out-of-range entries (oor_*), recurrent edges (rec_*): all with cfg = NULL"""
    import torch
    plan, image = M.build_case(CASES[name])
    want = M.gather_bytes(plan, image)
    assert not np.array_equal(want, image)
    _same_image(_gather(torch, plan, image), want, plan, name)


@pytest.mark.parametrize("name", ["oor_ff", "oor_rec"])
def test_rows_of_out_of_range_entries_keep_the_sentinel(name):
    import torch
    case = CASES[name]
    plan, image = M.build_case(case)
    rec = plan["mode"] == M.RECURRENT
    n_valid = 45 // plan["L"] if rec else 45
    entries = np.asarray(case["entries"], dtype=np.int64)
    assert (45 % plan["L"] != 0) == rec and plan["rows"] == len(entries)
    for e in (-1, n_valid, n_valid + 5, 2 ** 32 + 3, 2 ** 31, M.INT64_MAX, M.INT64_MIN):
        assert e in entries
    out = (entries < 0) | (entries >= n_valid)
    assert out.sum() == 8 and len(set(entries[~out].tolist())) < int((~out).sum())          # valid ones, some of them twice
    got = _gather(torch, plan, image)
    for i, f in enumerate(plan["fields"]):
        head = f["kind"] == M.CHUNK_HEAD
        rows = got[f["dst"]:f["dst"] + M.out_rows(plan, f["kind"]) * f["row_bytes"]].reshape(-1, f["row_bytes"])
        bad = np.tile(out, plan["L"] if rec and not head else 1)                             # row l * rows + k of chunk k, for every l; one head row per chunk
        assert rows.shape[0] == bad.size and (rows[bad] == M.SENTINEL).all(), (name, i)
        words = np.ascontiguousarray(rows[~bad]).view(np.uint32)
        assert not (words == M.SENTINEL * 0x01010101).any(), (name, i)                      # every other row was written, in every word
    _same_image(got, M.gather_bytes(plan, image), plan, name)                               # ... with the right bytes


# ---------------------------------------------------------------------- table kinds: the rows-form engine's own rows of the same rollout
TABLE_CONFIGS = {
    "july_E6_F8": dict(scenario_name=JULY, num_agents=3, world_size=2.4),                                        # E * E % 4 == 0: four entries per thread
    "nav_E7_F8": dict(scenario_name="navigation_graph", num_agents=3, num_obstacles=1, world_size=3.0),          # odd E: one entry per thread
    "rot_inv_E6_F7": dict(scenario_name=ROT_INV, num_agents=3, world_size=2.4),
    "nav_global_E7_F7": dict(scenario_name="navigation_graph", num_agents=3, num_obstacles=1, world_size=3.0, graph_feat_type="global"),
}
TABLE_T, TABLE_N = 4, 5
_rollouts = {}


def _rollout(torch, key):
    """a few steps of one config in the rows form and in the table form, the same actions: -> (cfg, NumPy obs, node_obs, adj of the rows form, entity table)"""
    if key not in _rollouts:
        from gmpe.engine import GmpeEngine
        from gmpe.rollout import DeviceRolloutBuffer
        kw = TABLE_CONFIGS[key]
        cfg = gmpe.make_config(num_envs=TABLE_N, episode_length=3, seed=41, **kw)          # episodes end inside the rollout
        engines = [GmpeEngine(cfg), GmpeEngine(cfg, adj_compact=True, node_form="table", adj_form="none")]
        bufs = [DeviceRolloutBuffer(e, TABLE_T) for e in engines]
        for b in bufs:
            b.warmup()
        if kw["scenario_name"] != "navigation_graph":
            _queue(engines[0], engines, np.random.RandomState(4), TABLE_N, cfg.num_agents)
        g = torch.Generator(device="cuda"); g.manual_seed(9)
        acts = torch.randint(0, cfg.n_actions, (TABLE_T, TABLE_N, cfg.num_agents), generator=g, device="cuda", dtype=torch.int32)
        for b in bufs:
            b.collect(acts)
        torch.cuda.synchronize()
        rows, tab = bufs
        assert rows._node_obs is not None and rows._adj is not None and rows._adj.dim() == 5 and tab._node_obs is None and tab._adj is None
        assert torch.equal(rows.obs, tab.obs) and int(rows.dones.sum()) > 0
        for e in engines:
            e.check_errors()
        _rollouts[key] = (cfg, rows.obs.cpu().numpy(), rows._node_obs.cpu().numpy(), rows._adj.cpu().numpy(), tab.entity_table.cpu().numpy())
    return _rollouts[key]


def _table_case(torch, key, recurrent, fields, seed):
    """fields: (kind, pad, dst_off) with kind "obs" (GMPE_MB_ROW), "node" or "adj" -> (cfg, plan, image before, image expected)"""
    cfg, obs, node, adj, table = _rollout(torch, key)
    T, N, A = TABLE_T, TABLE_N, cfg.num_agents
    E, F, W = cfg.num_entities, cfg.node_feats, cfg.entity_table_width
    assert obs.shape[:3] == (T + 1, N, A) and node.shape == (T + 1, N, A, E, F) and adj.shape == (T + 1, N, A, E, E) and table.shape == (T + 1, N, W)
    spec = dict(obs=(M.ROW, obs.shape[3] * 4, obs), node=(_lib.MB_TABLE_NODE, E * F * 4, node), adj=(_lib.MB_TABLE_ADJ, E * E * 4, adj))
    L = 7 if recurrent else 1                                                  # 60 % 7 != 0
    n_valid = T * N * A // L
    rng = np.random.RandomState(seed)
    entries = rng.randint(0, n_valid, 6 if recurrent else 23).astype(np.int64)
    entries[[1, 3, 4]] = (-1, 2 ** 32 + 3, n_valid)                            # out of range, among valid and duplicated entries
    rows, off = len(entries), 3
    laid, src0, size = M.layout(T, N, A, lambda kind: rows * L, [(spec[k][0], spec[k][1], pad, 0, do) for k, pad, do in fields], table_row=W * 8)
    perm = rng.randint(0, n_valid, off + max(rows, L) + 3).astype(np.int64)
    perm[off:off + rows] = entries
    plan = dict(mode=M.RECURRENT if recurrent else M.FEED_FORWARD, T=T, N=N, A=A, L=L, perm=perm, offset=off, rows=rows, fields=laid, src0=src0)
    image = np.full(size, M.SENTINEL, dtype=np.uint8)
    image[src0:] = M.source_bytes(seed + 1, size - src0)
    want = None
    for f, (k, pad, do) in zip(laid, fields):                                  # the sources, slot_stride apart
        src = obs if k == "obs" else table
        for t in range(T + 1):
            b = np.ascontiguousarray(src[t]).reshape(-1).view(np.uint8)
            image[f["src"] + t * f["slot_stride"]:f["src"] + t * f["slot_stride"] + b.size] = b
    want = image.copy()
    ok, t, n, a = M.row_samples(plan)
    assert ok.sum() == (rows - 3) * L
    for f, (k, pad, do) in zip(laid, fields):
        rb, arr = f["row_bytes"], spec[k][2]
        for r in np.flatnonzero(ok):
            want[f["dst"] + r * rb:f["dst"] + (r + 1) * rb] = np.ascontiguousarray(arr[t[r], n[r], a[r]]).reshape(-1).view(np.uint8)
    return cfg, plan, image, want


@pytest.mark.parametrize("recurrent", [False, True], ids=["ff", "rec"])
@pytest.mark.parametrize("key", sorted(TABLE_CONFIGS))
def test_table_kinds_equal_the_rows_form_engine(key, recurrent):
    import torch
    cfg = _rollout(torch, key)[0]
    E, F = cfg.num_entities, cfg.node_feats
    assert (E * E % 4 == 0) == (E == 6) and F == (8 if key.endswith("F8") else 7)
    node_offs = (0,) if F == 8 else (0, 4, 8, 12)                              # F = 8 rows are 16-byte vectors: another dst is refused (tests/test_minibatch_host.py)
    plans = {
        "aligned": [("obs", 0, 0), ("node", 0, 0), ("adj", 0, 0)],                                          # four entries per thread where E * E % 4 == 0
        "adj dst at 0, 4, 8, 12": [("adj", 0, do) for do in M.OFFSETS],
        "two adj fields, one at 4": [("adj", 0, 0), ("node", 0, 0), ("adj", 0, 4)],                        # the misaligned one takes both to one entry per thread
        "adj at 8 alone": [("adj", 0, 8)],
        "node rows by dst": [("node", 0, do) for do in node_offs],
        "slot + 8 bytes": [("adj", 8, 0), ("node", 8, 0), ("obs", 8, 4), ("adj", 0, 0)],
    }
    for i, (what, fields) in enumerate(plans.items()):
        cfg, plan, image, want = _table_case(torch, key, recurrent, fields, 300 + i)
        assert not np.array_equal(want, image)
        _same_image(_gather(torch, plan, image, cfg), want, plan, (key, what))


def test_table_kinds_need_the_config_they_are_given():
    """NULL is refused with a table kind in the plan, before any launch: the buffer stays as it was"""
    import torch
    cfg, plan, image, want = _table_case(torch, "july_E6_F8", False, [("adj", 0, 0)], 77)
    buf, perm = _upload(torch, plan, image)
    with pytest.raises(_lib.GmpeError, match="need a config"):
        _launch(torch, plan, buf, perm, None)
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy(), image)


# ---------------------------------------------------------------------- two calls, and a captured graph
def test_two_calls_into_two_destinations_give_identical_bytes():
    import torch
    cfg, tplan, timage, twant = _table_case(torch, "nav_E7_F8", True, [("obs", 8, 4), ("node", 0, 0), ("adj", 0, 4), ("adj", 8, 0)], 55)
    cplan, cimage = M.build_case(CASES["wl_255"])
    for plan, image, want, c in ((tplan, timage, twant, cfg), (cplan, cimage, M.gather_bytes(cplan, cimage), None)):
        a, perm = _upload(torch, plan, image)
        b = a.clone()
        assert a.data_ptr() != b.data_ptr() and b.data_ptr() % 256 == 0
        _launch(torch, plan, a, perm, c)
        _launch(torch, plan, b, perm, c)
        torch.cuda.synchronize()
        assert torch.equal(a, b)
        _same_image(a.cpu().numpy(), want, plan, "first call")


def test_the_call_is_capturable_in_a_graph():
    """copy and table kinds: two launches in series on one stream. The permutation is read at replay, so new contents give the new minibatch."""
    import torch
    fields = [("obs", 8, 4), ("node", 0, 0), ("adj", 0, 0), ("obs", 0, 0)]
    cfg, plan, image, want1 = _table_case(torch, "july_E6_F8", True, fields, 91)
    perm2 = plan["perm"][::-1].copy()
    perm2[plan["offset"] + 2] = M.INT64_MIN
    plan2 = dict(plan, perm=perm2)
    want2 = image.copy()
    ok, t, n, a = M.row_samples(plan2)
    _, obs, node, adj, _ = _rollout(torch, "july_E6_F8")
    for f, (k, pad, do) in zip(plan["fields"], fields):
        rb, arr = f["row_bytes"], dict(obs=obs, node=node, adj=adj)[k]
        for r in np.flatnonzero(ok):
            want2[f["dst"] + r * rb:f["dst"] + (r + 1) * rb] = np.ascontiguousarray(arr[t[r], n[r], a[r]]).reshape(-1).view(np.uint8)
    assert not np.array_equal(want1, want2)
    first = torch.from_numpy(image).cuda()
    eager, perm = _upload(torch, plan, image)
    captured = eager.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                              # one stream, no parallel branches
        _launch(torch, plan, captured, perm, cfg)
    for contents, want in ((plan["perm"], want1), (perm2, want2)):
        perm.copy_(torch.from_numpy(contents).cuda())                         # in place: the graph holds the pointer
        eager.copy_(first); captured.copy_(first)
        _launch(torch, plan, eager, perm, cfg)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, eager)
        _same_image(captured.cpu().numpy(), want, plan, "replay")
