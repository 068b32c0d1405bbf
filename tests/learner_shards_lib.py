"""Shared by tests/test_learner_shards_host.py and tests/test_gpu_learner_shards.py: the inputs, the splits into shards and a float64 NumPy emulation
of the two merge orders of the sharded learner statistics (include/gmpe.h gmpe_compute_returns_shard, gmpe_ppo_loss_shard).

Returns: a shard's (n, mean, M2) in the kernels' own order, then Chan's merge as a left fold over the shards in index order, then the float32 pair
(mean32, den32). returns_lib.kernel_order_stats gives only the rounded pair of one array, so shard_stat repeats its steps up to the triple with
returns_lib's own _chan and constants; tests/test_learner_shards_host.py pins it to kernel_order_stats on every shard (same pair, bit for bit).

PPO loss: a shard's double sums of returns, returns^2, active_masks and its row count, then a sequential sum over the shards in index order, then the
denominators and the float32 ValueNorm update from the global sums. The order of the sums inside a shard is not pinned bit for bit anywhere in the
suite (tests/test_gpu_ppo_loss.py holds the state within (log2(B) + 4) * U * mean|x|), so math.fsum stands in for it.

The wrong variants (VARIANTS_RETURNS, VARIANTS_LOSS) are what a sharded implementation gets wrong cheaply; the host test shows which input catches each."""
import math

import numpy as np

import ppo_loss_lib as P
import returns_lib as R

F32 = np.float32

# ------------------------------------------------------------------------------------------------ returns
# name -> (stat case or builder, path, lane counts of the shards). "+idle": a further shard whose entries are all inactive is appended.
IDLE_LANES = 70
PM100_LANES = (90, 40)


def _pm100():
    """Two shards with means near +100 and -100 (std 0.5 each), 90 and 40 lanes: the global mean is near 38, far from either shard's."""
    rng = np.random.RandomState(501)
    T, L = 9, sum(PM100_LANES)
    am = (rng.rand(T + 1, L) > 0.2).astype(F32)
    a = (0.5 * rng.randn(T, L)).astype(F32)
    a[:, :PM100_LANES[0]] += F32(100.0)
    a[:, PM100_LANES[0]:] -= F32(100.0)
    a = np.where(am[:T] != 0, a, (3.0 * rng.randn(T, L) + 1.0).astype(F32)).astype(F32)
    a[a == 0] = F32(0.25)
    return a, am


def _with_idle(a, am, copies=1, first=False):
    """`copies` shards of IDLE_LANES lanes with no active entry (ordinary values, active_masks 0) after (or before) the lanes of (a, am)."""
    rng = np.random.RandomState(502)
    T = a.shape[0]
    ia = (2.0 + rng.randn(T, IDLE_LANES * copies)).astype(F32)
    iam = np.zeros((T + 1, IDLE_LANES * copies), F32)
    parts_a, parts_m = ([ia, a], [iam, am]) if first else ([a, ia], [am, iam])
    return np.concatenate(parts_a, 1), np.concatenate(parts_m, 1)


def returns_case(name):
    """-> (adv [T, lanes], active_masks [T + 1, lanes], lane counts of the shards) of a prescribed-advantages case."""
    c = R.stat_cases()
    if name == "offset-65+65":
        return c["offset"] + ((65, 65),)
    if name == "unequal-1+128+64":
        return c["unequal"] + ((1, 128, 64),)
    if name == "nan-65+65":
        return c["nan"] + ((65, 65),)
    if name == "offset-130+idle":
        return _with_idle(*c["offset"]) + ((130, IDLE_LANES),)
    if name == "nan-130+idle":
        return _with_idle(*c["nan"]) + ((130, IDLE_LANES),)
    if name == "pm100-90+40":
        return _pm100() + (PM100_LANES,)
    if name == "idle+idle+offset":                            # host only: two empty shards first, where a merge without the empty-side shortcuts is 0 / 0
        return _with_idle(*c["offset"], copies=2, first=True) + ((IDLE_LANES, IDLE_LANES, 130),)
    raise KeyError(name)


RETURNS_CASES = ("offset-65+65", "unequal-1+128+64", "nan-65+65", "offset-130+idle", "nan-130+idle", "pm100-90+40")
HOST_ONLY_RETURNS_CASES = ("idle+idle+offset",)
PATHS = ("advantages", "recurrence")
BRANCH_T, BRANCH_SPLIT = 9, (65, 65)                           # the GAE x ValueNorm branch case: returns_lib.branch_inputs(9, 130)


def bounds(split):
    lo = np.concatenate([[0], np.cumsum(split)])
    return [(int(lo[i]), int(lo[i + 1])) for i in range(len(split))]


def shard_stat(adv, active_masks, ascending):
    """-> (n, mean, M2) float64 of one shard as gmpe_returns.hip forms it (the steps of returns_lib.kernel_order_stats, variant None, up to the merged
    Stat): Welford per lane over t, the 64-lane xor butterfly with the lower lane as the left operand, 256 strided accumulators, a halving tree."""
    a32 = R._rows(adv).astype(np.float32)
    T, lanes = a32.shape
    keep = (R._rows(active_masks, T) != 0) & ~np.isnan(a32)
    W = (lanes + R.WAVE - 1) // R.WAVE
    pad = lambda v: np.concatenate([v, np.zeros((T, W * R.WAVE - lanes), v.dtype)], 1)
    x, keep = pad(a32.astype(np.float64)), pad(keep)
    st = tuple(np.zeros(W * R.WAVE) for _ in range(3))
    with np.errstate(all="ignore"):
        for t in (range(T) if ascending else reversed(range(T))):
            n1 = st[0] + 1.0
            d = x[t] - st[1]
            m1 = st[1] + d / n1
            new = (n1, m1, st[2] + d * (x[t] - m1))
            st = tuple(np.where(keep[t], u, v) for u, v in zip(new, st))
    st = tuple(v.reshape(W, R.WAVE) for v in st)
    lane = np.arange(R.WAVE)
    off = 1
    while off < R.WAVE:
        o = tuple(v[:, lane ^ off] for v in st)
        lo, hi = R._chan(st, o), R._chan(o, st)
        st = tuple(np.where((lane & off) != 0, h, l) for l, h in zip(lo, hi))
        off <<= 1
    part = tuple(v[:, 0] for v in st)
    acc = tuple(np.zeros(R.STAT_THREADS) for _ in range(3))
    for r in range((W + R.STAT_THREADS - 1) // R.STAT_THREADS):
        chunk = tuple(v[r * R.STAT_THREADS:(r + 1) * R.STAT_THREADS] for v in part)
        k = chunk[0].size
        m = R._chan(tuple(v[:k] for v in acc), chunk)
        acc = tuple(np.concatenate([u, v[k:]]) for u, v in zip(m, acc))
    w = R.STAT_THREADS // 2
    while w > 0:
        acc = R._chan(tuple(v[:w] for v in acc), tuple(v[w:2 * w] for v in acc))
        w >>= 1
    return tuple(np.float64(v[0]) for v in acc)


def to_pair(stat):
    """(n, mean, M2) -> (mean32, den32): the tail of returns_lib.kernel_order_stats."""
    n, mean, m2 = stat
    if n == 0 or np.isnan(n):
        return F32(np.nan), F32(np.nan)
    with np.errstate(all="ignore"):
        return F32(mean), F32(F32(np.sqrt(np.fmax(m2, 0.0) / n)) + R.EPS32)


VARIANTS_RETURNS = ("unmerged", "mean_of_means", "empty_not_skipped")


def fold(stats, variant=None):
    """The shards' (n, mean, M2) -> the global one: Chan's merge as a left fold in index order, an empty side skipped. Wrong variants:
    unmerged: shard 0's own statistics; mean_of_means: the plain average of the shards' means and of their variances;
    empty_not_skipped: the merge formula with no shortcut for an empty side."""
    assert variant is None or variant in VARIANTS_RETURNS
    stats = [tuple(np.float64(x) for x in s) for s in stats]
    if variant == "unmerged":
        return stats[0]
    if variant == "mean_of_means":
        with np.errstate(all="ignore"):
            k = float(len(stats))
            mean = sum(s[1] for s in stats) / k
            var = sum(s[2] / s[0] for s in stats) / k
            n = sum(s[0] for s in stats)
            return n, mean, var * n
    s = stats[0]
    for b in stats[1:]:
        s = tuple(np.float64(v) for v in R._chan(s, b, shortcuts=variant != "empty_not_skipped"))
    return s


def emulate_returns(adv, active_masks, split, ascending, variant=None):
    """-> (mean32, den32) of the sharded call over the lanes of (adv, active_masks) split into `split` lane counts."""
    return to_pair(fold([shard_stat(adv[:, lo:hi], active_masks[:, lo:hi], ascending) for lo, hi in bounds(split)], variant))


# ------------------------------------------------------------------------------------------------ PPO loss
ROWS = 1030
LOSS_SPLITS = ((257, 773), (1, 256, 773))
LOSS_KS = (5, 25)
FAMILIES = dict(off_vn=dict(pm=False, vm=False, clipped=False, huber=False, valuenorm=True),
                on_vn=dict(pm=True, vm=True, clipped=True, huber=True, valuenorm=True),
                on_plain=dict(pm=True, vm=True, clipped=True, huber=True, valuenorm=False))
# (family, K, split, special): special None, "one_active" (every active row in shard 0) or "pm100" (returns near +100 in shard 0, near -100 elsewhere)
LOSS_CASES = [(f, K, s, None) for f in FAMILIES for K in LOSS_KS for s in LOSS_SPLITS] + \
             [("on_vn", 5, (257, 773), "one_active"), ("off_vn", 5, (257, 773), "one_active"), ("on_vn", 25, (257, 773), "pm100"),
              ("off_vn", 5, (257, 773), "pm100")]
# pm100 is not combined with the 1 + 256 + 773 split: one row near +100 among 1029 near -100 has mean^2 / var near 100, where ValueNorm's own float32
# msq - mean^2 cancels and the REFERENCE's float32 arithmetic is 175 units from float64 — outside what C_DEV (four times the reference's own error on
# well-conditioned returns) was derived for, sharded or not. tests/test_learner_shards_host.py asserts that every case here stays inside C_REF.
_LOSS = {}


def loss_case_id(case):
    return "%s-K%d-%s%s" % (case[0], case[1], "+".join(str(x) for x in case[2]), "-" + case[3] if case[3] else "")


def loss_case(case):
    """-> (inp, cfg, state, float64 restatement over the concatenated minibatch), made once. The special cases change a family's inputs; the rows of
    the result are still either exact ties or separated by ppo_loss_lib.MARGIN in every decision (other seeds are tried until they are), so that no row
    is ever left out of a comparison."""
    if case in _LOSS:
        return _LOSS[case]
    import torch
    fam, K, split, special = case
    c = P.cfg(**FAMILIES[fam])
    st = P.fresh_state() if c.use_valuenorm else None
    for seed in range(20):
        inp = P.family("generic", ROWS, K, seed=seed, c=c, state=st, masks="mixed", avail="given")
        if special == "one_active":
            m = np.zeros((ROWS, 1), F32)
            m[:split[0]:2] = 1.0
            inp["active_masks"] = m
        elif special == "pm100":
            shift = np.full((ROWS, 1), -100.0, F32)
            shift[:split[0]] = 100.0
            inp["returns"] = (inp["returns"] + shift).astype(F32)
        if special is None or not P.undecided(inp, c, st).any():
            break
    else:
        raise AssertionError("could not separate the decisions of %r" % (case,))
    _LOSS[case] = (inp, c, st, P.restate(inp, c, torch.float64, st))
    return _LOSS[case]


def rows_of(inp, lo, hi):
    return {k: (None if v is None else v[lo:hi]) for k, v in inp.items()}


def shard_sums(inp):
    """-> float64 [4]: sum returns, sum returns^2, sum active_masks, rows of one shard."""
    r = inp["returns"].astype(np.float64).reshape(-1)
    return np.array([math.fsum(r), math.fsum(r * r), math.fsum(inp["active_masks"].astype(np.float64).reshape(-1)), float(r.size)])


VARIANTS_LOSS = ("unmerged", "local_rows")


def global_sums(all_sums, variant=None, shard=0):
    """[world, 4] -> [4]: the rows added sequentially in index order. unmerged: shard `shard`'s own row; local_rows: the global sums with that
    shard's own row count (and so its own denominators where they are row counts)."""
    assert variant is None or variant in VARIANTS_LOSS
    all_sums = np.asarray(all_sums, np.float64)
    if variant == "unmerged":
        return all_sums[shard].copy()
    s = all_sums[0].copy()
    for row in all_sums[1:]:
        s = s + row
    if variant == "local_rows":
        s[3] = all_sums[shard][3]
    return s


def denominators(c, s):
    """(D_policy, D_value) from the global sums."""
    return (s[2] if c.use_policy_active_masks else s[3]), (s[2] if c.use_value_active_masks else s[3])


def valuenorm_update32(state, s, beta=0.99999):
    """ValueNorm.update from the global sums, float32 as the kernel's running_update: batch means rounded from double once."""
    bm, bsq = F32(s[0] / s[3]), F32(s[1] / s[3])
    b, w = F32(beta), F32(1.0 - beta)
    g = lambda k: F32(np.asarray(state[k]).reshape(-1)[0])
    return dict(running_mean=g("running_mean") * b + bm * w, running_mean_sq=g("running_mean_sq") * b + bsq * w, debiasing_term=g("debiasing_term") * b + w)


def state_tolerance(inp, k):
    """What tests/test_gpu_ppo_loss.py holds the unsharded call's ValueNorm state to."""
    B = len(inp["returns"])
    x = inp["returns"].astype(np.float64) ** 2 if k == "running_mean_sq" else inp["returns"].astype(np.float64)
    return (np.log2(B) + 4) * P.U * float(np.abs(x).mean()) if k != "debiasing_term" else 2 * P.U
