"""Float32 NumPy restatement of GraphReplayBuffer.compute_returns (onpolicy/utils/graph_buffer.py:285-366), GR_MAPPO.train's advantage lines
(onpolicy/algorithms/graph_mappo.py:294-304) and the runner's stop-action rule (graph_mpe_runner.py:73-141, 263-335), used by the tests to check
the device kernels at shapes the golden fixtures do not cover. It is pinned to the reference itself by tests/test_returns_host.py, which compares it
bit for bit with tests/golden/returns_advantages.npz and available_actions.npz (both made by running the reference)."""
import math

import numpy as np


def np_returns(rewards, masks, value_preds, returns, next_value, gamma, gae_lambda, use_gae, use_proper_time_limits, bad_masks=None, denorm=None):
    """-> (returns, value_preds) after compute_returns. The expressions keep the reference's operand order: a Python float meets a float32 array as
    float32(value), and gamma * gae_lambda is a double product rounded once. denorm: (mean, std) float32 scalars: x * std + mean, two roundings."""
    f32 = np.float32
    vp, ret = value_preds.astype(f32, copy=True), returns.astype(f32, copy=True)
    nv = next_value.astype(f32).reshape(vp.shape[1:])
    g, gl = f32(gamma), f32(gamma * gae_lambda)
    dn = (lambda x: x * f32(denorm[1]) + f32(denorm[0])) if denorm is not None else (lambda x: x)
    T = rewards.shape[0]
    if use_gae:
        vp[-1] = nv
        gae = np.zeros_like(nv)
        for s in reversed(range(T)):
            delta = rewards[s] + g * dn(vp[s + 1]) * masks[s + 1] - dn(vp[s])
            gae = delta + (gl * gae * masks[s + 1] if (use_proper_time_limits and denorm is not None) else gl * masks[s + 1] * gae)
            if use_proper_time_limits:
                gae = gae * bad_masks[s + 1]
            ret[s] = gae + dn(vp[s])
    else:
        ret[-1] = nv
        for s in reversed(range(T)):
            if use_proper_time_limits:
                ret[s] = (ret[s + 1] * g * masks[s + 1] + rewards[s]) * bad_masks[s + 1] + (f32(1) - bad_masks[s + 1]) * dn(vp[s])
            else:
                ret[s] = ret[s + 1] * g * masks[s + 1] + rewards[s]
    return ret, vp


def np_advantages(returns, value_preds, denorm=None):
    f32 = np.float32
    dv = value_preds[:-1] * f32(denorm[1]) + f32(denorm[0]) if denorm is not None else value_preds[:-1]
    return returns[:-1] - dv


def np_normalized(adv, active_masks):
    """(adv - mean) / (std + 1e-5) over the entries with active_masks != 0 (and not NaN), population std; statistics in double, as the kernels."""
    a = adv.astype(np.float64)
    keep = (active_masks[:-1] != 0) & ~np.isnan(a)
    if not keep.any():
        return np.full_like(adv, np.nan)
    m = a[keep].mean()
    sd = np.sqrt(((a[keep] - m) ** 2).mean())
    return (adv - np.float32(m)) / (np.float32(sd) + np.float32(1e-5))


def np_available_actions(dones, n_actions):
    """[T, ...lanes] dones -> [T, ...lanes, n_actions]: position t = ones at t = 0, else the stop row (one-hot at n_actions // 2) where dones[t - 1]."""
    out = np.ones(dones.shape + (n_actions,), np.float32)
    for t in range(1, dones.shape[0]):
        d = dones[t - 1].astype(bool)
        out[t][d] = 0.0
        out[t][d, n_actions // 2] = 1.0
    return out


# ------------------------------------------------------------------------------------------------ the advantage statistics, bit for bit
# k_adv_normalize is fdiv_rn(fsub_rn(a, mean32), den32): two correctly rounded float32 operations, as NumPy's float32 (adv - m) / d. Given the raw
# advantages (checked bit for bit on their own), the whole normalised array is a function of the pair (mean32, den32) alone, so it is compared bit for
# bit against the few pairs a correct double accumulation can end at, instead of within a tolerance.
F32 = np.float32
EPS32 = np.float32(1e-5)
N_MAX, KAPPA_MAX = 2 ** 16, 2.0 ** 10
M_OFFSETS, D_OFFSETS = (-1, 0, 1), (-2, -1, 0, 1, 2)


def _rows(x, T=None):
    x = np.asarray(x)
    x = x.reshape(x.shape[0], -1)
    return x if T is None else x[:T]


def _keep(adv, active_masks):
    a = _rows(adv).astype(np.float32)
    return a, (_rows(active_masks, a.shape[0]) != 0) & ~np.isnan(a)


def stats64(adv, active_masks):
    """-> (mean, std, n) of the entries with active_masks != 0 that are not NaN: float64, two passes with exactly rounded sums, population std.
    adv: [T, ...lanes]; active_masks: [T, ...] or [T + 1, ...] (the buffer's array, whose last slot is not read)."""
    a, keep = _keep(adv, active_masks)
    x = a[keep].astype(np.float64)
    if x.size == 0:
        return float("nan"), float("nan"), 0
    mean = math.fsum(x) / x.size
    return mean, math.sqrt(math.fsum((x - mean) ** 2) / x.size), int(x.size)


def _ulps(x, k):
    for _ in range(abs(k)):
        x = np.nextafter(x, F32(np.inf if k > 0 else -np.inf))
    return x


def candidate_pairs(mean64, std64, n):
    """-> [(dm, dd, mean32, den32)]: mean32 = float32(mean64) moved by dm in {-1, 0, 1} ulps, den32 = float32(float32(std64) + float32(1e-5)) moved by
    dd in {-2 .. 2} ulps. The widths are derived, not measured: a double Welford / Chan accumulation over n <= 2^16 entries has a relative error of
    at most n * 2^-53 * kappa in either statistic, kappa = rms / std for the std and rms / |mean| for the mean (rms = sqrt(mean^2 + var)). With
    kappa <= 2^10 that is < 2^-27, under a quarter of a float32 ulp, so rounding the kernel's double to float32 lands at most one ulp from the
    rounding of the exact value. For the denominator, + 1e-5f is one more rounding of two inputs one ulp apart: at most two ulps where the sum
    crosses a binade. The inputs must stay inside those limits; both are asserted here. n is stats64's count, passed along so that its limit can be
    asserted too. The limit on rms / |mean| means that data whose mean is zero (or below rms / 2^10) cannot use this criterion: its float32(mean)
    has no bounded relative error, so such an input needs an offset or an exact expectation of its own."""
    assert 2 <= n <= N_MAX, "n = %r is outside the derivation (2 .. 2^16)" % (n,)
    assert std64 > 0 and mean64 != 0, "a constant or zero-mean input has no condition number: give it an exact expectation of its own"
    rms = math.sqrt(mean64 * mean64 + std64 * std64)
    assert rms / std64 <= KAPPA_MAX and rms / abs(mean64) <= KAPPA_MAX, "kappa: rms / std = %.4g, rms / |mean| = %.4g exceed 2^10" % (
        rms / std64, rms / abs(mean64))
    m0, d0 = F32(mean64), F32(F32(std64) + EPS32)
    return [(dm, dd, _ulps(m0, dm), _ulps(d0, dd)) for dm in M_OFFSETS for dd in D_OFFSETS]


def _same_bits(x, y):
    """float32 arrays equal bit for bit, NaN positions compared as NaN (a NaN's payload and sign are not pinned)."""
    x, y = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)
    nx, ny = np.isnan(x), np.isnan(y)
    return x.shape == y.shape and bool((nx == ny).all()) and bool((x.view(np.uint32)[~nx] == y.view(np.uint32)[~nx]).all())


def normalize32(adv, mean32, den32):
    with np.errstate(all="ignore"):
        return (np.asarray(adv, np.float32) - F32(mean32)) / F32(den32)


def match_pair(adv_bits, normalized_bits, pairs):
    """-> (dm, dd) of the one candidate whose float32 (adv - m) / d is the device's normalised array bit for bit (NaN positions as NaN), or None if
    there is none. adv_bits / normalized_bits: uint32 views (or float32 arrays) of the device's raw and normalised advantages. An input on which
    two candidates give the same array cannot tell them apart and is refused."""
    adv = np.ascontiguousarray(adv_bits).view(np.float32)
    got = np.ascontiguousarray(normalized_bits).view(np.float32)
    hits = [(dm, dd) for dm, dd, m, d in pairs if _same_bits(normalize32(adv, m, d), got)]
    assert len(hits) <= 1, "candidates %r give the same array: the input does not discriminate" % (hits,)
    return hits[0] if hits else None


def pair_offsets(mean32, den32, pairs):
    """-> (dm, dd) of a (mean32, den32) pair inside the candidate set, or None (a NaN is never inside)."""
    for dm, dd, m, d in pairs:
        if F32(mean32) == m and F32(den32) == d:
            return dm, dd
    return None


# The kernel's own order in NumPy (float64 by default). The CPU stand-in for the kernel in tests/test_returns_host.py, where it and ten wrong variants
# of it show that the inputs below tell them apart; no GPU test compares against it.
WAVE, STAT_THREADS, CHUNK = 64, 256, 8
# Where this emulation lands among the candidates of every input below, in either order (asserted in tests/test_returns_host.py). It repeats the
# kernel's IEEE double operations one for one in the kernel's order (no contraction on either side, sqrt and division correctly rounded), so the
# device is held to the same pair.
KERNEL_ORDER_OFFSETS = (0, 0)
VARIANTS = ("float32", "naive32", "weight_b", "no_shortcuts", "ddof1", "nan_kept", "inactive_kept", "hi_partials_dropped", "last_wave_dropped",
            "tail_dropped")


def _chan(a, b, weight_b=False, shortcuts=True):
    (an, am, a2), (bn, bm, b2) = a, b
    with np.errstate(all="ignore"):
        n = an + bn
        f = bn / n
        d = bm - am
        out = (n, am + d * f, a2 + b2 + d * d * ((bn if weight_b else an) * f))
    if not shortcuts:
        return out
    return tuple(np.where(bn == 0, x, np.where(an == 0, y, z)) for x, y, z in zip(a, b, out))


def _add(a, b):
    return tuple(x + y for x, y in zip(a, b))


def kernel_order_stats(adv, active_masks, ascending=False, variant=None):
    """-> (mean32, den32) as gmpe_returns.hip forms them: Welford per lane over t (descending in k_returns, ascending=True for k_advantages), the
    64-lane xor butterfly with the lower lane as the left operand, the per-wave partials merged by 256 strided accumulators and a halving tree,
    then float32(mean) and float32(float32(sqrt(M2 / n)) + 1e-5f). variant: None, or one of VARIANTS (a wrong kernel)."""
    assert variant is None or variant in VARIANTS
    a32 = _rows(adv).astype(np.float32)
    T, lanes = a32.shape
    act = _rows(active_masks, T) != 0
    keep = act & ~np.isnan(a32)
    if variant == "nan_kept":
        keep = act
    if variant == "inactive_kept":
        keep = ~np.isnan(a32)
    W = (lanes + WAVE - 1) // WAVE
    if variant == "last_wave_dropped" and lanes % WAVE:
        keep[:, (W - 1) * WAVE:] = False
    if variant == "tail_dropped" and T % CHUNK:
        if ascending:
            keep[T - T % CHUNK:] = False
        else:
            keep[:T % CHUNK] = False
    dt = np.float32 if variant in ("float32", "naive32") else np.float64
    naive = variant == "naive32"
    merge = _add if naive else (lambda x, y: _chan(x, y, variant == "weight_b", variant != "no_shortcuts"))
    pad = lambda v: np.concatenate([v, np.zeros((T, W * WAVE - lanes), v.dtype)], 1)
    x, keep = pad(a32.astype(dt)), pad(keep)
    st = tuple(np.zeros(W * WAVE, dt) for _ in range(3))
    with np.errstate(all="ignore"):
        for t in (range(T) if ascending else reversed(range(T))):
            if naive:
                new = (st[0] + dt(1), st[1] + x[t], st[2] + x[t] * x[t])
            else:
                n1 = st[0] + dt(1)
                d = x[t] - st[1]
                m1 = st[1] + d / n1
                new = (n1, m1, st[2] + d * (x[t] - m1))
            st = tuple(np.where(keep[t], u, v) for u, v in zip(new, st))
    st = tuple(v.reshape(W, WAVE) for v in st)
    lane = np.arange(WAVE)
    off = 1
    while off < WAVE:
        o = tuple(v[:, lane ^ off] for v in st)
        lo, hi = merge(st, o), merge(o, st)
        st = tuple(np.where((lane & off) != 0, h, l) for l, h in zip(lo, hi))
        off <<= 1
    part = tuple(v[:, 0] for v in st)
    acc = tuple(np.zeros(STAT_THREADS, dt) for _ in range(3))
    for r in range(1 if variant == "hi_partials_dropped" else (W + STAT_THREADS - 1) // STAT_THREADS):
        chunk = tuple(v[r * STAT_THREADS:(r + 1) * STAT_THREADS] for v in part)
        k = chunk[0].size
        m = merge(tuple(v[:k] for v in acc), chunk)
        acc = tuple(np.concatenate([u, v[k:]]) for u, v in zip(m, acc))
    w = STAT_THREADS // 2
    while w > 0:
        acc = merge(tuple(v[:w] for v in acc), tuple(v[w:2 * w] for v in acc))
        w >>= 1
    n, s1, s2 = (v[0] for v in acc)
    if n == 0:
        return F32(np.nan), F32(np.nan)
    with np.errstate(all="ignore"):
        if naive:
            mean = s1 / n
            m2 = (s2 / n - mean * mean) * n
        else:
            mean, m2 = s1, s2
        den = n - dt(1) if variant == "ddof1" else n
        return F32(mean), F32(F32(np.sqrt(np.fmax(m2, dt(0)) / den)) + EPS32)


# The inputs of tests/test_gpu_returns_statistics.py: name -> (adv f32 [T, lanes], active_masks f32 [T + 1, lanes]), the smallest shapes at which each
# mechanism exists. tests/test_returns_host.py shows on the CPU that each wrong variant above leaves the candidate set on at least one of them.
CONST_VALUE = F32(0.1)
STEP_TS = (8, 9, 16, 17)
EXACT_CASES = ("const", "two_equal")          # fewer than two distinct active values: exact expectations instead of candidates
_CASES = {}


def _active(rng, T, lanes, p=0.2):
    am = (rng.rand(T + 1, lanes) > p).astype(np.float32)
    return am


def _build_cases():
    c = {}
    # mean ~ 100, std ~ 0.1: kappa ~ 10^3. Three waves, the last with 2 lanes. Inactive entries come from another distribution.
    rng = np.random.RandomState(101)
    T, L = 9, 130
    am = _active(rng, T, L)
    a = (100.0 + 0.1 * rng.randn(T, L)).astype(np.float32)
    a = np.where(am[:T] != 0, a, (5.0 * rng.randn(T, L)).astype(np.float32))
    c["offset"] = (a, am)
    # the same with another seed: on "offset" float32 accumulators happen to survive k_advantages' ascending order, here neither order lets them
    rng = np.random.RandomState(111)
    am = _active(rng, T, L)
    a = (100.0 + 0.1 * rng.randn(T, L)).astype(np.float32)
    a = np.where(am[:T] != 0, a, (5.0 * rng.randn(T, L)).astype(np.float32))
    c["offset2"] = (a, am)
    # unequal partial counts: wave 0 full N(0, 1); wave 1 one active entry (50); wave 2 none; wave 3 (1 lane) N(-3, 0.01)
    rng = np.random.RandomState(102)
    T, L = 9, 193
    a = rng.randn(T, L).astype(np.float32)
    am = np.zeros((T + 1, L), np.float32)
    am[:, :64] = 1.0
    a[:, 64:192] = (7.0 + rng.randn(T, 128)).astype(np.float32)
    am[4, 64 + 37] = 1.0
    a[4, 64 + 37] = 50.0
    am[:, 192] = 1.0
    a[:, 192] = (-3.0 + 0.1 * rng.randn(T)).astype(np.float32)
    c["unequal"] = (a, am)
    # NaN at >= 10 % of the active entries; inactive entries hold 1e30, +-inf, NaN and ordinary values
    rng = np.random.RandomState(103)
    T, L = 9, 130
    am = _active(rng, T, L)
    a = (1.0 + rng.randn(T, L)).astype(np.float32)
    a[(rng.rand(T, L) < 0.15) & (am[:T] != 0)] = np.nan
    junk = np.array([1e30, np.inf, -np.inf, np.nan, -4.0, 12.5], np.float32)
    a = np.where(am[:T] != 0, a, junk[rng.randint(0, len(junk), (T, L))])
    c["nan"] = (a, am)
    # 258 partials: 0 .. 255 ~ N(0, 1e-3), 256 and 257 near 10: the second round of the strided merge decides the result
    rng = np.random.RandomState(104)
    T, L = 2, 64 * 257 + 5
    am = _active(rng, T, L)
    a = (np.sqrt(1e-3) * rng.randn(T, L)).astype(np.float32)
    a[:, 64 * 256:] = (10.0 + 0.5 * rng.randn(T, L - 64 * 256)).astype(np.float32)
    a = np.where(am[:T] != 0, a, (3.0 + rng.randn(T, L)).astype(np.float32))
    c["tail_partial"] = (a, am)
    # rollout lengths at and around the unroll factor: step t scaled by 2^(t mod 5) around its own offset, so a missed or doubled step shows
    for T in STEP_TS:
        rng = np.random.RandomState(200 + T)
        L = 65
        am = _active(rng, T, L)
        t = np.arange(T)[:, None]
        a = ((rng.randn(T, L) + 0.5 + 0.25 * t) * 2.0 ** (t % 5)).astype(np.float32)
        a = np.where(am[:T] != 0, a, (-20.0 + rng.randn(T, L)).astype(np.float32))
        c["steps%d" % T] = (a, am)
    # every active advantage the same float32; inactive ones differ
    rng = np.random.RandomState(105)
    T, L = 9, 130
    am = _active(rng, T, L)
    a = np.where(am[:T] != 0, CONST_VALUE, rng.randn(T, L).astype(np.float32)).astype(np.float32)
    c["const"] = (a, am)
    # two active entries with equal values in different waves
    rng = np.random.RandomState(106)
    T, L = 3, 70
    a = rng.randn(T, L).astype(np.float32)
    am = np.zeros((T + 1, L), np.float32)
    am[1, 3] = am[2, 66] = 1.0
    a[1, 3] = a[2, 66] = CONST_VALUE
    c["two_equal"] = (a, am)
    for a, am in c.values():
        assert a.dtype == np.float32 and am.dtype == np.float32 and not (a == 0).any()        # no zero: -0.0 would not survive R = 0 + a
        a.setflags(write=False)
        am.setflags(write=False)
    return c


def stat_cases():
    if not _CASES:
        _CASES.update(_build_cases())
    return _CASES


def prescribed_inputs(adv, path):
    """Inputs of gmpe_compute_returns whose raw advantages are `adv` [T, lanes] exactly -> dict of float32 arrays [T(+1), lanes, 1].
    "advantages": returns = adv, value_preds = 0 (k_advantages: adv - 0). "recurrence": use_gae=False, masks = 0, rewards = adv, value_preds = 0
    (k_returns: R = (R' * gamma * 0) + adv, then R - 0). A non-finite entry would poison the earlier steps of its lane there (NaN * 0), so it goes
    in through value_preds instead: reward 0 and value_pred -adv give 0 - (-adv). So on this path the `a == a` filter of k_returns meets only
    NaNs that arise in R - v0d from value_preds (R = 0); a NaN return is filtered on the advantages-only path alone."""
    T, L = adv.shape
    z = lambda n: np.zeros((n, L, 1), np.float32)
    a = adv.reshape(T, L, 1)
    if path == "advantages":
        ret = z(T + 1)
        ret[:T] = a
        return dict(returns=ret, value_preds=z(T + 1))
    assert path == "recurrence"
    fin = np.isfinite(a)
    vp = z(T + 1)
    vp[:T] = np.where(fin, np.float32(0), -a)
    return dict(rewards=np.where(fin, a, np.float32(0)), masks=z(T + 1), value_preds=vp, returns=z(T + 1), next_value=np.zeros((L, 1), np.float32))


# The inputs of the all-branches tests (GAE x proper time limits x denormaliser, random masks): shared so that tests/test_returns_host.py can show on
# the CPU that their advantages stay inside candidate_pairs' limits.
DENORM = (np.float32(0.37), np.float32(1.9))
BRANCH_LANES = 65


def branch_inputs(T, lanes=BRANCH_LANES, seed=None):
    rng = np.random.RandomState(300 + T if seed is None else seed)
    f32 = np.float32
    return dict(rewards=rng.randn(T, lanes, 1).astype(f32), value_preds=rng.randn(T + 1, lanes, 1).astype(f32),
                masks=(rng.rand(T + 1, lanes, 1) > 0.1).astype(f32), bad_masks=(rng.rand(T + 1, lanes, 1) > 0.05).astype(f32),
                active_masks=(rng.rand(T + 1, lanes, 1) > 0.2).astype(f32), returns=rng.randn(T + 1, lanes, 1).astype(f32),
                next_value=rng.randn(lanes, 1).astype(f32))


def branch_expectations(d, gae, proper, denorm):
    """-> (returns, value_preds, raw advantages) of one branch of compute_returns on branch_inputs' arrays."""
    ret, vp = np_returns(d["rewards"], d["masks"], d["value_preds"], d["returns"], d["next_value"], 0.99, 0.95, gae, proper, d["bad_masks"], denorm)
    return ret, vp, np_advantages(ret, vp, denorm)
