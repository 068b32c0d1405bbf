"""NumPy restatement of the minibatch gather (include/gmpe.h gmpe_minibatch_gather): the reference's sampler arithmetic (graph_buffer.py:385-399, 617-622) and
the two index maps from an output row to its sample (t, n, a). tests/test_minibatch_host.py checks it against the reference's own yields
(tests/golden/minibatch_generators.npz); the GPU tests compare the kernel with it. Below the shaped form: the byte-level form (gather_bytes on a uint8 image of
device memory: byte offsets, padded strides, unwritten rows) and KERNEL_CASES, from which tests/test_minibatch_host.py and tests/test_gpu_minibatch_kernel.py draw."""
import numpy as np

NAMES = ("share_obs", "obs", "node_obs", "adj", "agent_id", "share_agent_id", "rnn_states", "rnn_states_critic", "actions", "value_preds", "returns", "masks",
         "active_masks", "action_log_probs", "advantages", "available_actions")


def ff_sampler(T, N, A, num_mini_batch=None, mini_batch_size=None):
    batch = N * T * A
    if mini_batch_size is None:
        mini_batch_size = batch // num_mini_batch
    return [(i * mini_batch_size, max(0, min(batch, (i + 1) * mini_batch_size) - i * mini_batch_size)) for i in range(num_mini_batch)]


def rec_sampler(T, N, A, num_mini_batch, L):
    chunks = N * T * A // L
    mbc = chunks // num_mini_batch
    return [(i * mbc, mbc) for i in range(num_mini_batch)]


def ff_samples(perm, off, rows, T, N, A):
    """output row r -> j = perm[off + r] over the [T, N, A] flattening"""
    j = np.asarray(perm[off:off + rows], dtype=np.int64)
    return j // (N * A), (j // A) % N, j % A


def rec_samples(perm, off, chunks, T, N, A, L):
    """output row r = l * chunks + k -> f = perm[off + k] * L + l in the [N, A, T] order; and the chunk heads (l = 0)"""
    c = np.asarray(perm[off:off + chunks], dtype=np.int64)
    f = (c[None, :] * L + np.arange(L)[:, None]).reshape(-1)
    dec = lambda f: ((f % T), f // (A * T), (f // T) % A)
    return dec(f), dec(c * L)


def gather(arrays, t, n, a, centralized, heads=None):
    """the 16 arrays of one minibatch from [T+1, N, A, ...] arrays (materialised adjacency) at samples (t, n, a); heads: (t, n, a) of the rnn rows"""
    o = {}
    obs, ids = arrays["obs"], arrays["agent_id"]
    o["share_obs"] = obs[t, n].reshape(len(t), -1) if centralized else obs[t, n, a]
    o["share_agent_id"] = ids[t, n].reshape(len(t), -1) if centralized else ids[t, n, a]
    for k in ("obs", "node_obs", "adj", "agent_id", "actions", "value_preds", "returns", "masks", "active_masks", "action_log_probs", "advantages",
              "available_actions"):
        o[k] = arrays[k][t, n, a] if arrays.get(k) is not None else None
    ht, hn, ha = (t, n, a) if heads is None else heads
    for k in ("rnn_states", "rnn_states_critic"):
        o[k] = arrays[k][ht, hn, ha]
    return o


# ---------------------------------------------------------------------- the byte-level form (header comment of gmpe_minibatch_gather, include/gmpe.h)
# A plan here is a dict: mode, T, N, A, L, perm (int64 array), offset, rows, fields; a field is a dict: kind, row_bytes, slot_stride, src, dst, the last two byte
# offsets into one uint8 image of device memory whose base is 256-byte aligned. The table kinds are not restated: their rows come from the engine.
FEED_FORWARD, RECURRENT = 0, 1
ROW, ENV_ROW, CHUNK_HEAD = 0, 1, 2
MAX_FIELDS = 20
BLOCK = 256                                   # threads of one workgroup: for the coverage asserts and the `>` wrong variant only, never for an expected byte
SENTINEL = 0xA5
ROW_SIZES = (4, 8, 12, 16, 20, 32, 48, 100, 1040)
OFFSETS = (0, 4, 8, 12)
PADS = (0, 4, 8, 16)
INT64_MAX, INT64_MIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min


class Header(object):
    """The rules the header documents, one method each; tests/test_minibatch_host.py overrides one at a time to make the wrong restatements."""

    def valid_count(self, samples, L, recurrent):
        return samples // L if recurrent else samples

    def entry(self, e):                       # the int64 entry as compared with the range
        return e

    def in_range(self, e, n_valid):
        return (e >= 0) & (e < n_valid)

    def split(self, r, rows):                 # recurrent output row r = l * rows + k -> (k, l)
        return r % rows, r // rows

    def head_l(self, rows):                   # a chunk head is the chunk's first sample
        return 0

    def ff_tna(self, j, T, N, A):
        return j // (N * A), (j // A) % N, j % A

    def row_index(self, kind, n, a, A):
        return n if kind == ENV_ROW else n * A + a

    def stride(self, field, slot):
        return field["slot_stride"]

    def unwritten_prefix(self, plan, i):      # leading bytes of field i's output that no thread writes
        return 0


HEADER = Header()


def unit_width(field):
    """the unit the documented rule selects for a copy field: 16, 8 or 4 bytes from the OR of src, dst, slot_stride and row_bytes"""
    al = field["src"] | field["dst"] | field["slot_stride"] | field["row_bytes"]
    return 16 if al % 16 == 0 else (8 if al % 8 == 0 else 4)


def out_rows(plan, kind):
    return plan["rows"] * plan["L"] if plan["mode"] == RECURRENT and kind != CHUNK_HEAD else plan["rows"]


def field_threads(plan, field):
    """threads of a copy field: output rows * units per row"""
    return out_rows(plan, field["kind"]) * (field["row_bytes"] // unit_width(field))


def row_samples(plan, head=False, rules=HEADER, trace=None):
    """per output row (per chunk with head): ok (entry in range), t, n, a"""
    T, N, A = plan["T"], plan["N"], plan["A"]
    rec = plan["mode"] == RECURRENT
    L = plan["L"] if rec else 1
    perm, off, rows = np.asarray(plan["perm"], dtype=np.int64), plan["offset"], plan["rows"]
    n_valid = rules.valid_count(T * N * A, L, rec)
    if not rec or head:
        k = np.arange(rows, dtype=np.int64)
        l = np.full(rows, rules.head_l(rows) if rec else 0, dtype=np.int64)
    else:
        k, l = rules.split(np.arange(rows * L, dtype=np.int64), rows)
    if trace is not None:
        trace["perm_max"] = max(trace.get("perm_max", -1), int((off + k).max()))
    e = rules.entry(perm[off + k])
    ok = rules.in_range(e, n_valid)
    e = np.where(ok, e, 0)
    if rec:
        f = e * L + l
        t, n, a = f % T, f // (A * T), (f // T) % A
    else:
        t, n, a = rules.ff_tna(e, T, N, A)
    return ok, t, n, a


def gather_bytes(plan, memory, rules=HEADER, trace=None):
    """The image of device memory after gmpe_minibatch_gather(plan) from the image before it: whole rows copied, rows of out-of-range entries and every other
    byte kept. trace (a dict) receives the extent of the source bytes and permutation entries read."""
    N, A = plan["N"], plan["A"]
    out = memory.copy()
    for i, f in enumerate(plan["fields"]):
        kind, rb = f["kind"], f["row_bytes"]
        if kind not in (ROW, ENV_ROW, CHUNK_HEAD):
            raise ValueError("the table kinds are not restated here")
        ok, t, n, a = row_samples(plan, kind == CHUNK_HEAD, rules, trace)
        slot = rb * (N if kind == ENV_ROW else N * A)
        src = f["src"] + t * rules.stride(f, slot) + rules.row_index(kind, n, a, A) * rb
        for r in np.flatnonzero(ok):
            s, d = int(src[r]), f["dst"] + int(r) * rb
            if trace is not None:
                trace["src_min"], trace["src_max"] = min(trace.get("src_min", s), s), max(trace.get("src_max", 0), s + rb)
            out[d:d + rb] = memory[s:s + rb]
        keep = min(rules.unwritten_prefix(plan, i), len(ok) * rb)
        out[f["dst"]:f["dst"] + keep] = memory[f["dst"]:f["dst"] + keep]
    return out


def _up(x, a=256):
    return -(-x // a) * a


def layout(T, N, A, rows_of, fields, table_row=None):
    """Byte offsets of one image: destinations first, a guard of at least 256 bytes before, between and behind them, then the sources, T + 1 slots each, then
    slack that a wrong row map may read without leaving the image. fields: (kind, row_bytes, pad, src_off, dst_off): slot_stride is one slot + pad, src and dst
    lie src_off / dst_off bytes past a 256-byte boundary. table_row: the source row bytes of the table kinds (W * 8). -> (field dicts, first source byte, size)"""
    out, cur = [], 256
    for kind, rb, pad, so, do in fields:
        out.append(dict(kind=kind, row_bytes=rb, dst=cur + do))
        cur = _up(cur + do + rows_of(kind) * rb) + 256
    src0, slack = cur, 0
    for f, (kind, rb, pad, so, do) in zip(out, fields):
        slot = table_row * N if kind > CHUNK_HEAD else rb * (N if kind == ENV_ROW else N * A)
        f["slot_stride"], f["src"] = slot + pad, cur + so
        cur = _up(cur + so + (T + 1) * (slot + pad))
        slack = max(slack, (A + 2) * (T + 1) * (slot + pad))
    return out, src0, cur + slack


def source_bytes(seed, n):
    """n random bytes (n % 4 == 0) none of whose aligned 4-byte words is the sentinel word"""
    w = np.random.RandomState(seed).randint(0, 1 << 32, n // 4, dtype=np.uint64).astype(np.uint32)
    w[w == SENTINEL * 0x01010101] ^= 1
    return w.view(np.uint8)


def build_case(case):
    """-> (plan, image before the call): destinations and guards hold the sentinel, everything from the first source byte on is random"""
    T, N, A = case["tna"]
    rec = case["mode"] == RECURRENT
    L = case["L"] if rec else 1
    rows, off = case["rows"], case["offset"]
    fields, src0, size = layout(T, N, A, lambda kind: rows if kind == CHUNK_HEAD or not rec else rows * L, case["fields"])
    n_valid = T * N * A // L
    rng = np.random.RandomState(case["seed"])
    perm = rng.randint(0, n_valid, off + max(rows, L) + 3).astype(np.int64)    # duplicates included; entries past the minibatch are valid too
    if case.get("entries") is not None:
        perm[off:off + rows] = np.asarray(case["entries"], dtype=np.int64)
    image = np.full(size, SENTINEL, dtype=np.uint8)
    image[src0:] = source_bytes(case["seed"] + 1, size - src0)
    plan = dict(mode=case["mode"], T=T, N=N, A=A, L=L, perm=perm, offset=off, rows=rows, fields=fields, src0=src0)
    return plan, image


def _kernel_cases():
    cases = []

    def add(name, mode, tna, fields, rows, L=1, offset=2, entries=None):
        assert 1 <= len(fields) <= MAX_FIELDS and all(rb in ROW_SIZES and pad in PADS for _, rb, pad, _, _ in fields), name
        cases.append(dict(name=name, seed=1000 + 7 * len(cases), mode=mode, tna=tna, fields=fields, rows=len(entries) if entries is not None else rows, L=L,
                          offset=offset, entries=entries))

    base, big = (3, 5, 3), (5, 9, 6)
    # alignments and strides: every (src, dst) offset pair, each with one of the strides so that every src and every dst offset meets every stride; each row
    # size, both modes, per-sample and per-env-step rows; chunk heads in the recurrent plans, which then have MAX_FIELDS fields
    for mode, mname in ((FEED_FORWARD, "ff"), (RECURRENT, "rec")):
        for kind, kname in ((ROW, "row"), (ENV_ROW, "env_row")):
            for rb in ROW_SIZES:
                fields = [(kind, rb, PADS[(i + j) % 4], so, do) for i, so in enumerate(OFFSETS) for j, do in enumerate(OFFSETS)]
                if mode == RECURRENT:
                    fields += [(CHUNK_HEAD, rb, PADS[j], OFFSETS[j], OFFSETS[(j + 1) % 4]) for j in range(4)]
                add("align_%s_%s_%d" % (mname, kname, rb), mode, base, fields, 13 if mode == FEED_FORWARD else 5, 4)
    # each unit width because of one quantity alone: the other three are multiples of 16
    add("widths_alone", FEED_FORWARD, base, [(ROW, 16, 0, 0, 0), (ROW, 16, 0, 8, 0), (ROW, 16, 0, 4, 0), (ROW, 16, 0, 12, 0), (ROW, 16, 0, 0, 8), (ROW, 16, 0, 0, 4),
                                             (ROW, 16, 0, 0, 12), (ROW, 16, 8, 0, 0), (ROW, 16, 4, 0, 0), (ROW, 8, 8, 0, 0), (ROW, 4, 4, 0, 0), (ROW, 1040, 0, 0, 0)], 17)
    # out-of-range entries among valid and duplicated ones
    mixed = [(ROW, 20, 4, 0, 0), (ENV_ROW, 48, 0, 8, 0), (ROW, 1040, 0, 0, 0), (ENV_ROW, 4, 8, 0, 4), (ROW, 16, 16, 0, 8)]
    bad = lambda n: [7, -1, n, 7, n + 5, 2 ** 32 + 3, 2 ** 31, INT64_MAX, INT64_MIN, n - 1, 0, 3, 2 ** 32 + 3, 5]
    add("oor_ff", FEED_FORWARD, base, mixed, None, entries=bad(45))
    add("oor_rec", RECURRENT, base, mixed + [(CHUNK_HEAD, 12, 0, 0, 4), (CHUNK_HEAD, 32, 4, 8, 0)], None, 4, entries=bad(11))        # 45 % 4 != 0: the count is the floor
    # the work list: MAX_FIELDS fields, one-workgroup fields, 255 / 256 / 257 threads, several workgroups; a one-workgroup field between two large ones
    H = CHUNK_HEAD
    wl = [(ROW, 48, 0, 4, 0), (H, 4, 0, 0, 0), (ENV_ROW, 100, 4, 0, 0), (ROW, 4, 0, 0, 0), (H, 20, 0, 0, 4), (ROW, 16, 0, 0, 0), (H, 16, 0, 0, 0), (ROW, 100, 0, 0, 8),
          (ROW, 8, 0, 0, 0), (ROW, 8, 0, 0, 4), (H, 8, 8, 0, 0), (ENV_ROW, 32, 0, 8, 0), (H, 48, 0, 0, 0), (ENV_ROW, 4, 0, 0, 0), (ROW, 12, 4, 0, 0), (H, 12, 0, 4, 0),
          (ROW, 20, 0, 0, 0), (ENV_ROW, 16, 16, 0, 0), (H, 32, 0, 0, 12), (ROW, 32, 0, 12, 0)]
    ff_wl = [(ROW if k == H else k, rb, pad, so, do) for k, rb, pad, so, do in wl]
    for name, mode, fields, rows, L in (("wl_255", RECURRENT, wl, 51, 5), ("wl_256", RECURRENT, wl, 64, 4), ("wl_257", FEED_FORWARD, ff_wl, 257, 1),
                                        ("wl_257_rec", RECURRENT, wl, 1, 257)):
        add(name, mode, big, fields, rows, L)
        add(name + "_reversed", mode, big, fields[::-1], rows, L)
    add("single", FEED_FORWARD, base, [(ROW, 20, 0, 0, 0)], 9)
    # recurrent edges
    edge = [(ROW, 20, 4, 0, 0), (ENV_ROW, 48, 0, 8, 0), (CHUNK_HEAD, 12, 0, 0, 4), (ROW, 16, 0, 0, 0)]
    add("rec_L1", RECURRENT, base, edge, 7, 1)
    add("rec_LT", RECURRENT, base, edge, 6, 3)
    add("rec_L7", RECURRENT, base, edge, 4, 7)                              # L > T and 45 % 7 != 0
    add("rec_A1", RECURRENT, (3, 5, 1), edge, 3, 2)
    add("rec_N1", RECURRENT, (3, 1, 3), edge, 3, 2)
    add("rec_rows1", RECURRENT, base, edge, 1, 4)
    return cases


KERNEL_CASES = _kernel_cases()
