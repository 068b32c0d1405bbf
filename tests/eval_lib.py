"""NumPy restatement of the batched evaluator (include/gmpe.h gmpe_episode_record / _metrics / _summary) — test helper, not a conftest.

Written from the rules, not from the kernels: per-episode columns with 1-D np.mean / np.sum per episode (what the render loop calls), order
statistics with np.percentile / np.median / np.min / np.max, and the success statistics over the flattened [episodes, A] 0/1 matrix.
"""
import numpy as np

COLUMNS = ["reward", "frac", "success", "collisions", "fairness", "dist_mean", "time_mean", "time_fairness", "stddev_param",
           "time_stddev_param", "total_dists_traveled", "total_time_taken", "conformance", "delta_space", "spacing_violations", "steps"]
STATS = ["min", "p10", "median", "p90", "max", "mean", "std"]
KEYS = ["individual_reward", "Dist_to_goal", "Time_req_to_goal", "Num_agent_collisions", "Num_obst_collisions", "Distance_mean",
        "Distance_variance", "Mean_by_variance", "Dists_traveled", "Time_taken", "Time_mean", "Time_stddev", "Time_mean_by_stddev",
        "Conformance", "Delta_spacing", "Spacing_violations", "Min_time_to_goal", "Phase_reached"]
K = {k: i for i, k in enumerate(KEYS)}


def cut_episodes(did_reset, T):
    """The render loop's break rule on a recorded rollout: (first step, length) of each complete episode."""
    s, segs = 0, []
    while True:
        e = next((t for t in range(s, min(s + T, len(did_reset))) if did_reset[t]), s + T - 1)
        if e >= len(did_reset):
            return segs
        segs.append((s, e - s + 1))
        s = e + 1


class Record(object):
    """Per-env record state driven step by step, as gmpe_episode_record defines it."""

    def __init__(self, N, A, T, n_actions=25, width=18, dtype=np.float32):
        self.N, self.A, self.T, self.n_actions = N, A, T, n_actions
        self.live = np.ones(N, bool)
        self.steps = np.zeros(N, np.int32)
        self.ret = np.zeros((N, A), np.float64)
        self.final_info = np.zeros((N, A, width), dtype)
        self.t = 0

    def step(self, reward, done, info):
        """reward [N, A] (the engine's f32, widened), done bool [N, A], info [N, A, W]; returns (masks [N, A, 1], available_actions [N, A, n_actions])."""
        done = np.asarray(done, bool)
        all_done = done.all(axis=1)
        lv = self.live.copy()
        self.ret[lv] = self.ret[lv] + np.asarray(reward)[lv].astype(np.float64)
        fin = lv & (all_done | (self.t == self.T - 1))
        self.final_info[fin] = info[fin]
        self.steps[fin] = self.t + 1
        self.live[fin] = False
        self.t += 1
        masks = np.ones((self.N, self.A, 1), np.float32)
        masks[done] = 0.0
        masks[all_done] = 1.0
        avail = np.ones((self.N, self.A, self.n_actions), np.float32)
        stop = np.zeros(self.n_actions, np.float32)
        stop[self.n_actions // 2] = 1.0
        avail[masks[..., 0] == 0] = stop
        return masks, avail


def episode_columns(final_info, ret, steps, T, dt, min_dist_thresh):
    """f64 [N, len(COLUMNS)] from the records (final_info as recorded, widened to f64)."""
    fi = np.asarray(final_info).astype(np.float64)
    N, A = fi.shape[:2]
    tdt = T * dt
    out = np.zeros((N, len(COLUMNS)))
    for n in range(N):
        f = fi[n]
        ttg = [tdt if v == -1 else v for v in f[:, K["Time_req_to_goal"]].tolist()]
        coll = 0
        for a in range(A):
            coll += f[a, K["Num_agent_collisions"]] / 2.0
            coll += f[a, K["Num_obst_collisions"]]
        last = f[A - 1]
        out[n] = [np.mean(ret[n]), np.max([v / tdt for v in ttg]), np.mean([int(v < min_dist_thresh) for v in f[:, K["Dist_to_goal"]]]), coll,
                  last[K["Mean_by_variance"]], last[K["Distance_mean"]], last[K["Time_mean"]], last[K["Time_mean_by_stddev"]],
                  1.0 / (last[K["Distance_variance"]] + 0.0001), 1.0 / (last[K["Time_stddev"]] + 0.0001), np.sum(f[:, K["Dists_traveled"]].tolist()),
                  np.sum(ttg), np.mean(f[:, K["Conformance"]].tolist()), np.mean(f[:, K["Delta_spacing"]].tolist()),
                  np.mean(f[:, K["Spacing_violations"]].tolist()), steps[n]]
    return out


def agent_sums(final_info, T, dt):
    """The render loop's dists_trav_list / time_taken_list: per-agent sums over the episodes."""
    fi = np.asarray(final_info).astype(np.float64)
    ttg = fi[..., K["Time_req_to_goal"]]
    ttg = np.where(ttg == -1, T * dt, ttg)
    return fi[..., K["Dists_traveled"]].sum(axis=0), ttg.sum(axis=0)


def stats_of(x):
    x = list(np.asarray(x).tolist())
    return {"min": np.min(x), "p10": np.percentile(x, 10), "median": np.median(x), "p90": np.percentile(x, 90), "max": np.max(x),
            "mean": np.mean(x), "std": np.std(x)}


def summary_stats(cols, A):
    """{column: {statistic: value}}; success over the flattened [N, A] 0/1 matrix the render loop keeps (success_rates_arr)."""
    cols = np.asarray(cols)
    out = {c: stats_of(cols[:, i]) for i, c in enumerate(COLUMNS)}
    counts = np.rint(cols[:, COLUMNS.index("success")] * A).astype(np.int64)
    flat = [[1] * int(c) + [0] * int(A - c) for c in counts]
    out["success"] = stats_of(np.array(flat))
    return out


# ----------------------------------------------------------------------------------------------------------------------------------------------
# Synthetic inputs, exact references and derived bounds for the three kernels driven directly (tests/test_gpu_eval_kernels.py); the inputs are
# proven sharp on the CPU in tests/test_eval_kernel_inputs_host.py.
# ----------------------------------------------------------------------------------------------------------------------------------------------
import decimal  # noqa: E402
import math  # noqa: E402
import warnings  # noqa: E402
from fractions import Fraction  # noqa: E402
from functools import lru_cache  # noqa: E402

U = Fraction(1, 2 ** 53)                 # unit roundoff of float64
ORDER_STATS = ["min", "p10", "median", "p90", "max"]
SUMMARY_NS = [1, 2, 3, 4, 5, 7, 8, 10, 11, 16, 17, 101, 255, 256, 257, 512, 1000, 4097, 100003]
SUMMARY_WIDTHS = [1, 5, 16, 64]          # num_columns of the tables of SUMMARY_NS[i]: SUMMARY_WIDTHS[i % 4]; 100 003 rows get 16 columns
SUCCESS_AGENTS = [1, 3, 10, 64]
# gamma = frac((n - 1) * 0.1) of np.percentile(., 10), in tenths, per n (p90 mirrors it); asserted in the host module
GAMMA_P10_TENTHS = {1: 0, 2: 1, 3: 2, 4: 3, 5: 4, 7: 6, 8: 7, 10: 9, 11: 0, 16: 5, 17: 6, 101: 0, 255: 4, 256: 5, 257: 6, 512: 1, 1000: 9,
                    4097: 6, 100003: 2}


def quiet(f, *a, **k):
    """f(*a, **k) with NumPy's inf / NaN warnings off: the non-finite families are expected to produce them."""
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        return f(*a, **k)


def width_of(n):
    return SUMMARY_WIDTHS[SUMMARY_NS.index(n) % 4]


def _bits(x):
    return np.asarray(x, np.float64).view(np.int64)


def low_bytes_needed(n):
    """Low bytes that must vary for n doubles under one shared prefix whose neighbours in value are at least 13 ulps apart (slots of 16 ulps):
    1 up to 16 rows, 2 up to 4096, else 3."""
    return 1 if n <= 16 else 2 if n <= 4096 else 3


def _low_byte_column(rng, n, nbytes, base, distinct, spaced=False):
    b = int(_bits(base)) & ~((1 << (8 * nbytes)) - 1)
    span = (1 << (8 * nbytes)) // (16 if spaced else 1)
    low = rng.permutation(span)[:n] if distinct else np.concatenate([rng.permutation(span) for _ in range(n // span + 1)])[:n]
    if spaced:
        low = low * 16 + rng.randint(0, 4, n)
    return (b + low.astype(np.int64)).view(np.float64)


def nan_rows(n):
    return [r for r in sorted({0, 255, 256, n - 1}) if r < n]


def success_shaped(rng, n, A):
    """Rows k / A for integer k in [0, A]: what k_episode_metrics leaves in the success column."""
    return rng.randint(0, A + 1, n).astype(np.float64) / A


@lru_cache(maxsize=None)
def summary_columns(n):
    """[(family name, f64 [n])]: one column per input family of gmpe_episode_summary for a table of n rows (success_column = -1 families).

    randn full-mantissa mixed sign; lowbyte(.neg) share their top 7 bytes and differ in the lowest byte alone (distinct up to 256 rows, tied
    beyond): the last radix pass alone decides every rank. Doubles that share 7 bytes are 256 consecutive ulps, and NumPy's interpolation
    between two neighbours one ulp apart rounds onto one of them, so this column cannot also tell the percentile methods apart; lowbytes does:
    all rows distinct, at least 13 ulps between neighbours, under the longest shared prefix that allows it (the lowest byte alone up to 16
    rows, low_bytes_needed(n) bytes beyond); ties3 three values, most rows equal; equal one
    value; zeros -0.0 and +0.0 with a few small values either side, every inner rank on a zero; subnormal; large (about 1e150, squares finite);
    inf1 / inf2 one +inf / both infs among randn; nan@r exactly one NaN at row r; f32w(.pos) f32 values widened (low 29 bits zero); kA the
    success column's k / A rows summarised as an ordinary column. Columns past the family list (wide tables) are re-seeded randn / lowbyte /
    f32w / large copies named "<family>#k"."""
    rng = np.random.RandomState(1000 + n)
    cols = [("randn", rng.randn(n))]
    cols.append(("lowbyte", _low_byte_column(rng, n, 1, 1.2345, n <= 256)))
    cols.append(("lowbyte.neg", _low_byte_column(rng, n, 1, -77.125, n <= 256)))
    cols.append(("lowbytes", _low_byte_column(rng, n, low_bytes_needed(n), 3.0e-7, True, spaced=True)))
    cols.append(("ties3", rng.choice([-1.5, 0.25, 7.0], size=n, p=[0.8, 0.15, 0.05])))
    cols.append(("equal", np.full(n, 0.1)))
    z = np.where(rng.rand(n) < 0.5, -0.0, 0.0)
    idx = rng.permutation(n)
    k = n // 12
    z[idx[:k]] = -np.abs(rng.randn(k)) * 1e-3
    z[idx[k:2 * k]] = np.abs(rng.randn(k)) * 1e-3
    cols.append(("zeros", z))
    cols.append(("subnormal", rng.randint(1 << 48, 1 << 51, n).astype(np.int64).view(np.float64)))
    cols.append(("large", rng.randn(n) * 1e150))
    x = rng.randn(n)
    x[rng.randint(n)] = np.inf
    cols.append(("inf1", x))
    if n >= 2:
        x = rng.randn(n)
        i, j = rng.permutation(n)[:2]
        x[i], x[j] = np.inf, -np.inf
        cols.append(("inf2", x))
    for r in nan_rows(n):
        x = rng.randn(n)
        x[r] = np.nan
        cols.append(("nan@%d" % r, x))
    cols.append(("f32w", (rng.rand(n) * 4 - 1).astype(np.float32).astype(np.float64)))
    cols.append(("f32w.pos", (rng.rand(n) * 4 + 0.5).astype(np.float32).astype(np.float64)))
    cols.append(("kA", success_shaped(rng, n, SUCCESS_AGENTS[SUMMARY_NS.index(n) % 4])))
    C = width_of(n)
    k = 0
    while len(cols) % C:
        k += 1
        f = k % 4
        x = rng.randn(n) if f == 1 else _low_byte_column(rng, n, 1, 1e10 * k, n <= 256) if f == 2 else \
            (rng.randn(n) * 3).astype(np.float32).astype(np.float64) if f == 3 else rng.randn(n) * 1e150
        cols.append(("%s#%d" % (["large", "randn", "lowbyte", "f32w"][f], k), x))
    for _, x in cols:
        x.setflags(write=False)
    return cols


def sharp_columns(n):
    """Full-mantissa, lowest-bytes (the spaced, distinct variant) and f32-widened columns at n rows: the inputs of the host sharpness tests."""
    d = dict(summary_columns(n))
    return {"randn": d["randn"], "lowbytes": d["lowbytes"], "f32w": d["f32w"]}


@lru_cache(maxsize=None)
def summary_tables(n):
    """The gmpe_episode_summary launches at n rows: [dict(table f64 [n, C], names [C] (None: filler, not a case), success_column, success_agents)].

    First the family columns of summary_columns(n) in chunks of C = width_of(n) with success_column = -1. Then six tables with a success column
    (its name "succ.A<a>@<pos>"): success_agents 1, 3, 10, 64 with the column first, in the middle or last (rotating with n, so the twelve
    combinations all occur), an all-zero and an all-one column; the other columns of those tables are family columns again, as filler."""
    cols = summary_columns(n)
    C = width_of(n)
    out = []
    for s in range(0, len(cols), C):
        chunk = cols[s:s + C]
        out.append(dict(table=np.ascontiguousarray(np.stack([x for _, x in chunk], 1)), names=[m for m, _ in chunk], success_column=-1,
                        success_agents=0))
    rng = np.random.RandomState(5000 + n)
    i = SUMMARY_NS.index(n)
    kinds = [(A, "rand") for A in SUCCESS_AGENTS] + [(SUCCESS_AGENTS[i % 4], "zero"), (SUCCESS_AGENTS[(i + 1) % 4], "one")]
    for j, (A, kind) in enumerate(kinds):
        pos = [0, C // 2, C - 1][(i + j) % 3]
        tab = np.stack([cols[(j + c) % len(cols)][1] for c in range(C)], 1).copy()
        tab[:, pos] = success_shaped(rng, n, A) if kind == "rand" else float(kind == "one")
        names = [None] * C
        names[pos] = "succ.A%d@%s%s" % (A, ["first", "mid", "last"][(i + j) % 3], "" if kind == "rand" else "." + kind)
        out.append(dict(table=tab, names=names, success_column=pos, success_agents=A))
    return out


def summary_cases():
    """[(n, table index, column index, name)] of every named column: the parametrised ids of the summary test."""
    return [(n, ti, ci, name) for n in SUMMARY_NS for ti, t in enumerate(summary_tables(n)) for ci, name in enumerate(t["names"]) if name]


def success_flat_stats(col, A):
    """summary_stats' flattened 0/1 matrix for one success column."""
    counts = np.rint(np.asarray(col) * A).astype(np.int64)
    x = (np.arange(A)[None, :] < counts[:, None]).astype(np.int64)           # row i: counts[i] ones, then zeros
    return {"min": np.min(x), "p10": np.percentile(x, 10), "median": np.median(x), "p90": np.percentile(x, 90), "max": np.max(x),
            "mean": np.mean(x), "std": np.std(x)}


def exact_moments(x):
    """(mean, population variance, sum |x|) of finite doubles as exact Fractions (integer arithmetic on the scaled mantissas)."""
    m, e = np.frexp(np.asarray(x, np.float64))
    emin = int(e.min()) - 53
    ints = [a << b for a, b in zip((m * float(1 << 53)).astype(np.int64).tolist(), (e - 53 - emin).tolist())]
    n, S, Q, Ab = len(ints), sum(ints), sum(v * v for v in ints), sum(abs(v) for v in ints)
    sc = Fraction(2) ** emin
    return Fraction(S, n) * sc, Fraction(n * Q - S * S, n * n) * sc * sc, Fraction(Ab) * sc


def _dec(fr, prec=60):
    with decimal.localcontext() as ctx:
        ctx.prec = prec
        return decimal.Decimal(fr.numerator) / decimal.Decimal(fr.denominator)


def check_mean_std(x, mean, std, moments=None):
    """Assert a mean and a population std computed in float64, in any summation order with a two-pass variance, against exact arithmetic.

    Bounds (u = 2^-53, first order, no overflow / underflow: finite columns in the normal range only):
    mean: n - 1 additions in any order give |s^ - s| <= (n - 1) u sum|x_i|; dividing by n adds one more rounding, inside the slack of n for
      n - 1. So |mean^ - mean| <= n u sum|x_i| / n = u sum|x_i| =: delta_max.
    std: each fl(x_i - m^) is rounded relative to its own result, squaring adds one rounding, the n - 1 additions of non-negative terms at
      most (n - 1) u, the division one: the computed sum of squares over n is within (n + 3) u of sum (x_i - m^)^2 / n, and
      sum (x_i - m^)^2 = sum (x_i - m)^2 + n delta^2 exactly (delta = m^ - m). So var^ = (var + delta^2) (1 + e), |e| <= (n + 3) u, and by
      sqrt(1 + t) <= 1 + t / 2 the std is within ((n + 3) u + delta_max^2 / var) / 2 of the exact one, plus 2 u for the sqrt's own rounding and
      this bound's first-order terms. With var = 0 the same steps give the absolute form std^ <= delta_max (1 + (n + 3) u / 2 + 2 u)."""
    m, var, sabs = moments or exact_moments(x)
    n = len(x)
    dmax = U * sabs
    assert math.isfinite(mean) and math.isfinite(std), (mean, std)
    err = abs(Fraction(mean) - m)
    assert err <= dmax, "mean %r: error %.3e above the bound u sum|x| = %.3e (exact mean %.17g)" % (mean, float(err), float(dmax), float(m))
    rel = ((n + 3) * U) / 2 + 2 * U
    if var == 0:
        bound = dmax * (1 + rel)
        assert 0 <= Fraction(std) <= bound, "std %r of a zero-variance column above the bound %.3e" % (std, float(bound))
        return float(err), float(Fraction(std)), float(bound)
    bound = rel + dmax * dmax / var / 2
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        ref = _dec(var).sqrt()
        got = abs(decimal.Decimal(std) - ref) / ref
        assert got <= _dec(bound), "std %r: relative error %.3e above the bound %.3e (exact std %.17g)" % (std, float(got), float(_dec(bound)), float(ref))
    return float(err), float(got), float(bound)


def numpy_agreement(x, moments=None):
    """(mean, std): whether float64 NumPy and the kernel must agree within rtol 1e-12 on this column ("well-conditioned").

    Both sum with at most D roundings on any path: the kernel ceil(n / 256) per thread plus an 8-level tree, NumPy's pairwise_sum 16 per
    unrolled block of 128 plus ceil(log2 n) levels, 2 for the divisions. Their means differ by at most D u sum|x| / n, their stds (two-pass in
    both) by at most ((D + 6) u + 2 (D u sum|x| / n)^2 / var) / 2 + 4 u relatively; the 1e-12 check applies where these a-priori figures are below it."""
    m, var, sabs = moments or exact_moments(x)
    n = len(x)
    D = -(-n // 256) + 8 + 16 + max(n - 1, 1).bit_length() + 2
    dm = D * U * sabs / n
    tol = Fraction(1, 10 ** 12)
    mean_ok = dm <= tol * abs(m)
    std_ok = var > 0 and ((D + 6) * U + 2 * dm * dm / var) / 2 + 4 * U <= tol
    return bool(mean_ok), bool(std_ok)


def is_normal_finite(x):
    x = np.asarray(x)
    return bool(np.all(np.isfinite(x)) and np.all((x == 0) | (np.abs(x) >= np.finfo(np.float64).tiny)))


# --- cheap wrong variants of the order statistics: the host module shows the inputs tell each of them from the truth

def stats_by_order(x, order, lerp_both=True):
    """The five order statistics of x read through a given ordering (a permutation of its rows), NumPy's linear rule."""
    s = np.asarray(x)[order]
    n = len(s)

    def pct(q):
        v = (n - 1) * (q / 100.0)
        lo = min(int(math.floor(v)), n - 1)
        hi = min(lo + 1, n - 1)
        g = v - math.floor(v)
        a, b = s[lo], s[hi]
        return b - (b - a) * (1 - g) if g >= 0.5 else a + (b - a) * g
    med = s[n // 2] if n % 2 else (s[n // 2 - 1] + s[n // 2]) / 2.0
    return [s[0], pct(10.0), med, pct(90.0), s[n - 1]]


def key_of(x):
    """The kernel's order-preserving u64 key of a double."""
    b = np.asarray(x, np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))


def kernel_np_sum(v):
    """Python transcription of the kernel's np_sum (NumPy's pairwise_sum below 128 values) on a list of floats."""
    n = len(v)
    if n < 8:
        r = -0.0
        for x in v:
            r += x
        return r
    r = list(v[:8])
    i = 8
    while i < n - (n % 8):
        for j in range(8):
            r[j] += v[i + j]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    while i < n:
        res += v[i]
        i += 1
    return res


def sequential_sum(v):
    r = 0.0
    for x in v:
        r += x
    return r


# --- gmpe_episode_metrics

METRIC_AGENTS = [1, 2, 7, 8, 9, 15, 16, 17, 24, 31, 32, 33, 63, 64]
METRIC_ENVS = [1, 255, 256, 257, 1000]
METRIC_T, METRIC_DT = 25, 0.1
METRIC_THRESH = float(np.float32(0.05))        # a double that an f32 Dist_to_goal can equal exactly
ROW_PATTERNS = ["all -1", "none -1", "nan first", "nan middle", "nan last", "mix", "mix", "mix"]
SUMMED = [("total_dists_traveled", "Dists_traveled", False), ("conformance", "Conformance", True), ("delta_space", "Delta_spacing", True),
          ("spacing_violations", "Spacing_violations", True)]


def row_pattern(i, A):
    """Time_req_to_goal pattern of env row i (shifted with the agent count, so that the one row of N = 1 meets every pattern across them)."""
    return ROW_PATTERNS[(i + METRIC_AGENTS.index(A)) % len(ROW_PATTERNS)]


@lru_cache(maxsize=None)
def metrics_inputs(N, A):
    """(final_info f32 [N, A, 18], ret f64 [N, A], steps i32 [N]) for gmpe_episode_metrics.

    ret is full-mantissa randn * 3. The info columns summed over agents are f32 values at four scales (2^0, 2^-31, 2^-33, 2^-36; |randn| * 2^k
    for Dists_traveled, randn * 2^k for the three means): f32 values of one magnitude add exactly in f64 and would hide the order of the sum. Time_req_to_goal is -1 or
    a step count times dt by row_pattern, with one NaN in the first / a middle / the last agent's entry in the NaN rows. A quarter of Dist_to_goal
    is exactly METRIC_THRESH; the last agent's Distance_variance / Time_stddev are -0.0001f in every fourth row."""
    rng = np.random.RandomState(77 * N + A)
    fi = (rng.rand(N, A, 18) * 4 - 1).astype(np.float32)
    wide = lambda: np.float32(2.0) ** rng.choice([0, -31, -33, -36], (N, A)).astype(np.float32)
    fi[..., K["Dists_traveled"]] = np.abs(rng.randn(N, A)).astype(np.float32) * wide()
    for k in ("Conformance", "Delta_spacing", "Spacing_violations"):
        fi[..., K[k]] = rng.randn(N, A).astype(np.float32) * wide()
    t = (rng.randint(1, METRIC_T + 1, (N, A)) * np.float32(METRIC_DT)).astype(np.float32)
    minus = rng.rand(N, A) < 0.5
    for i in range(N):
        p = row_pattern(i, A)
        if p == "all -1":
            minus[i] = True
        elif p == "none -1":
            minus[i] = False
    t[minus] = -1.0
    for i in range(N):
        p = row_pattern(i, A)
        if p.startswith("nan"):
            t[i, {"nan first": 0, "nan middle": A // 2, "nan last": A - 1}[p]] = np.nan
    fi[..., K["Time_req_to_goal"]] = t
    d = fi[..., K["Dist_to_goal"]] * np.float32(0.05)
    d[rng.rand(N, A) < 0.25] = np.float32(0.05)
    d[::3, 0] = np.float32(0.05)
    fi[..., K["Dist_to_goal"]] = d
    fi[..., K["Num_agent_collisions"]] = rng.randint(0, 7, (N, A))
    fi[..., K["Num_obst_collisions"]] = rng.randint(0, 4, (N, A))
    fi[1::4, A - 1, K["Distance_variance"]] = np.float32(-0.0001)
    fi[3::4, A - 1, K["Time_stddev"]] = np.float32(-0.0001)
    ret = rng.randn(N, A) * 3
    steps = rng.randint(1, METRIC_T + 1, N).astype(np.int32)
    for a in (fi, ret, steps):
        a.setflags(write=False)
    return fi, ret, steps


def check_sums(got, terms, divide_by=1, label=""):
    """Assert float64 sums over the last axis of `terms` (any order), then divided by `divide_by`, against math.fsum.

    n - 1 additions in any order are within (n - 1) u sum|x| of the exact sum and math.fsum within u |sum| of it, so |got - fsum| <= n u sum|x|
    (over divide_by; the division's rounding is second to the slack of the real error against this bound). A NaN term makes the sum NaN."""
    terms = np.asarray(terms, np.float64)
    got = np.asarray(got, np.float64)
    nan = np.isnan(terms).any(axis=-1)
    assert (np.isnan(got) == nan).all(), "%s: NaN sums %r, NaN terms %r" % (label, np.isnan(got).nonzero(), nan.nonzero())
    clean = np.where(nan[..., None], 0.0, terms)
    exact = np.array([math.fsum(r) for r in clean.reshape(-1, clean.shape[-1]).tolist()]).reshape(nan.shape) / divide_by
    bound = terms.shape[-1] * float(U) * np.abs(clean).sum(axis=-1) / divide_by
    err = np.where(nan, 0.0, np.abs(np.where(nan, 0.0, got) - exact))
    bad = err > bound
    assert not bad.any(), "%s: sums %r against math.fsum %r, errors %r above the bounds %r" % (label, got[bad], exact[bad], err[bad], bound[bad])


# --- gmpe_episode_record

RECORD_SHAPES = [(1, 1), (15, 64), (16, 64), (17, 64), (33, 5), (1000, 3), (4099, 10)]
RECORD_ACTIONS = [1, 2, 24, 25, 4096]
RECORD_RNN_ROWS = [None, 1, 7, 64, 1025]
RECORD_STEPS = [1, 2, 25]
DONE_PATTERNS = ["never", "all at one step", "one by one", "finished at step 0", "only by the last step"]


def record_cases():
    """[(N, A, n_actions, rnn_row, T)]: every shape with every action count (4096 actions at N <= 33) and every episode length; the RNN row
    width rotates through RECORD_RNN_ROWS so that each width meets each shape."""
    out = []
    for i, (N, A) in enumerate(RECORD_SHAPES):
        for j, na in enumerate(RECORD_ACTIONS):
            if na == 4096 and N > 33:
                continue
            for k, T in enumerate(RECORD_STEPS):
                out.append((N, A, na, RECORD_RNN_ROWS[(i + j + 2 * k) % 5], T))
    return out


def done_schedule(rng, pattern, A, T):
    """bool [T, A] dones of one env. never: no agent ever done. all at one step: all agents at one step (not the last, when T > 1). one by one:
    agents finish in a random order, one per step and stay done, the last at min(A, T) - 1 or later (the all-done row must come out all ones).
    finished at step 0: all done at step 0, random rows after. only by the last step: some agents done, never all."""
    d = np.zeros((T, A), bool)
    if pattern == "all at one step":
        d[rng.randint(0, max(T - 1, 1))] = True
    elif pattern == "one by one":
        order = rng.permutation(A)
        for t in range(T):
            d[t, order[:min(A, (t + 1) * -(-A // max(T - 1, 1)))]] = True
    elif pattern == "finished at step 0":
        d[:] = rng.rand(T, A) < 0.5
        d[0] = True
    elif pattern == "only by the last step":
        d[:] = rng.rand(T, A) < 0.5
        d[np.arange(T), rng.randint(0, A, T)] = False
    return d


def record_inputs(N, A, T, seed, pattern=None):
    """(reward f32 [T, N, A], done bool [T, N, A], info f32 [T, N, A, 18]); env i follows DONE_PATTERNS[(i + seed) % 5] unless `pattern` is given.
    info holds NaNs (two payloads) and -0.0 among random values."""
    rng = np.random.RandomState(seed)
    rew = (rng.randn(T, N, A) * 3).astype(np.float32)
    done = np.zeros((T, N, A), bool)
    for i in range(N):
        done[:, i] = done_schedule(rng, pattern or DONE_PATTERNS[(i + seed) % 5], A, T)
    info = (rng.rand(T, N, A, 18) * 4 - 1).astype(np.float32)
    r = rng.rand(T, N, A, 18)
    iv = info.view(np.int32)
    iv[r < 0.05] = 0x7fc00000
    iv[(r >= 0.05) & (r < 0.1)] = np.int32(-4079307)          # 0xffc1c0f5: a NaN with the sign bit and a payload
    iv[(r >= 0.1) & (r < 0.15)] = np.int32(-2 ** 31)          # -0.0
    return rew, done, info
