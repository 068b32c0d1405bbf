"""Shared by tests/test_act_host.py, tests/test_gpu_act.py and tests/test_gpu_act_buffer.py: the host restatement of the rollout half of the action
head (include/gmpe.h gmpe_act_sample), its input families, and the action stream's draws.

Restated lines: ACTLayer.forward for a Discrete head (onpolicy/algorithms/utils/act.py:107-113) = Categorical.forward (distributions.py:84-91: logits
at finfo(float32).min where available_actions == 0; torch's Categorical: l = x - logsumexp(x), probs = softmax(l)), mode() = probs.argmax (:27-28) or
sample(), log_probs (:18-25). The kernel's own rule replaces torch's sampler: c_j = the running sum of p_j over the available j in index order, the
action is the first available j with c_j > u, else the mode; u is one Philox draw per row, keyed by (seed, env, agent, draw). restate() does these steps
in float32 (NumPy, one rounding per operation, sums in index order) or in float64 (the yardstick). tests/test_act_host.py pins the float32 one to the
reference's own run (tests/golden/act_head.npz).

A row is AMBIGUOUS when u lies within (K + 4) * 2**-23 of a float64 CDF boundary: a float32 running sum of K probabilities, each rounded once after an
exp and a division, may differ from the float64 one by about that much, so float32 and float64 may pick either of the two actions next to the boundary.
"""
import numpy as np

FMIN32 = float(np.finfo(np.float32).min)
TOP = 1 << 63
M64 = (1 << 64) - 1
AMBIGUOUS_MAX = 0.005          # share of rows that may be ambiguous


def draws(seed, env_id_base, num_agents, draw, rows, row0=0):
    """u of the rows row0 .. row0 + rows - 1 of a batch whose row 0 is agent 0 of env env_id_base: the engine's Philox stream with the top counter bit."""
    import oracle_lib as ol                # binds the package: the fixture generator, which needs no draws, does without it
    lib = ol.load()
    A = int(num_agents)
    out = np.empty(rows, np.float64)
    for i in range(rows):
        r = row0 + i
        out[i] = lib.gmpo_philox_uniform(int(seed) & M64, (int(env_id_base) + r // A) & 0xFFFFFFFF, TOP | ((int(draw) * A + r % A) & M64))
    return out


def _seqsum(a):
    """Running sums along axis 1 in index order, one rounding per addition in a's dtype."""
    out = np.empty_like(a)
    acc = np.zeros(a.shape[0], a.dtype)
    for j in range(a.shape[1]):
        acc = acc + a[:, j]
        out[:, j] = acc
    return out


def restate(logits, avail=None, u=None, dtype=np.float32):
    """logits float32 [B, K]; avail [B, K] (non-zero = available) or None; u float64 [B] or None (mode only). Returns a dict: mode, actions (sampled, when u
    is given), log_probs of both, l (normalised logits), p, cdf (running sums over the sampling set; entries outside the set repeat the sum so far), set."""
    x = np.asarray(logits, np.float32).astype(dtype)
    B, K = x.shape
    av = np.ones((B, K), bool) if avail is None else (np.asarray(avail) != 0)
    x = np.where(av, x, dtype(FMIN32))
    with np.errstate(over="ignore", under="ignore"):
        m = x.max(axis=1, keepdims=True)
        s = _seqsum(np.exp(x - m))[:, -1:]
        lse = np.log(s) + m
        ml = m - lse
        l = x - lse
        e2 = np.exp(l - ml)
        s2 = _seqsum(e2)[:, -1:]
        p = e2 / s2
    sset = np.where(av.any(axis=1, keepdims=True), av, True)             # nothing available: the uniform row over all K
    mode = np.argmax(np.where(sset, x, -np.inf), axis=1)                 # the first index of the largest masked logit
    cdf = _seqsum(np.where(sset, p, dtype(0)))
    rows = np.arange(B)
    out = dict(mode=mode, mode_log_probs=l[rows, mode], l=l, p=p, cdf=cdf, set=sset)
    if u is not None:
        hit = sset & (cdf.astype(np.float64) > np.asarray(u, np.float64)[:, None])
        a = np.where(hit.any(axis=1), np.argmax(hit, axis=1), mode)
        out.update(actions=a, log_probs=l[rows, a])
    return out


def ambiguity(ref64, u, K):
    """(ambiguous [B] bool, allowed [B, K] bool) from the float64 restatement: a row is ambiguous when u is within (K + 4) * 2**-23 of a CDF boundary of its
    sampling set; it may then take either action next to that boundary (the mode stands in beyond the last one). Other rows may only take the float64 action."""
    sset, cdf = ref64["set"], ref64["cdf"]
    B = len(u)
    eps = (K + 4) * 2.0 ** -23
    near = sset & (np.abs(cdf - np.asarray(u)[:, None]) <= eps)
    allowed = np.zeros((B, K), bool)
    allowed[np.arange(B), ref64["actions"]] = True
    for r in np.nonzero(near.any(axis=1))[0]:
        idx = np.nonzero(sset[r])[0]
        for j in np.nonzero(near[r])[0]:
            allowed[r, j] = True
            nxt = idx[idx > j]
            allowed[r, nxt[0] if len(nxt) else ref64["mode"][r]] = True
    return near.any(axis=1), allowed


def family(name, B, K, seed=0, avail="mixed"):
    """Inputs of one family: logits float32 [B, K] uniform in +-1 ("unit") or +-30 ("wide": the max subtraction matters, most of the mass on few actions);
    avail: "none" | "mixed" (row index mod 5: all available, a stop row at K // 2, random 70 %, random 70 %, a single random action) |
    "empty" (as mixed, with every 7th row holding no available action at all)."""
    rng = np.random.RandomState(seed * 7919 + B * 31 + K + (0 if name == "unit" else 1000003))
    scale = 1.0 if name == "unit" else 30.0
    logits = ((rng.rand(B, K) * 2.0 - 1.0) * scale).astype(np.float32)
    if avail == "none":
        return logits, None
    av = (rng.rand(B, K) < 0.7).astype(np.float32)
    av[np.arange(B), rng.randint(0, K, B)] = 1.0                          # at least one
    k = np.arange(B) % 5
    av[k == 0] = 1.0
    av[k == 1] = 0.0
    av[k == 1, K // 2] = 1.0
    one = k == 4
    av[one] = 0.0
    av[one, rng.randint(0, K, int(one.sum()))] = 1.0
    if avail == "empty":
        av[np.arange(B) % 7 == 3] = 0.0
    return logits, av


def ulps32(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.maximum(np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64), 1e-45)


def lse_units(got, want, x_a, l64_a):
    """|got - want| of a log-prob in units of ulp32(max(|lse|, |l|)), lse = x_a - l from the float64 restatement: a log-prob is x_a - lse, so it carries the
    rounding of the logsumexp, which is coarser than its own ulp when the log-prob is near zero."""
    l64 = np.asarray(l64_a, np.float64)
    lse = np.asarray(x_a, np.float64) - l64
    unit = np.spacing(np.maximum(np.maximum(np.abs(lse), np.abs(l64)), 1e-30).astype(np.float32)).astype(np.float64)
    return np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)) / unit


# the cases the GPU suite runs and over which the host suite bounds the ambiguous rows: (family, rows, K, num_agents, env_id_base, avail)
CASES = [("unit", 1, 5, 3, 0, "mixed"), ("wide", 63, 25, 3, 7, "mixed"), ("unit", 257, 4, 10, 0, "mixed"), ("wide", 257, 5, 3, 1000, "empty"),
         ("unit", 1030, 25, 10, 123456, "mixed"), ("wide", 1030, 64, 3, 5, "mixed"), ("unit", 1030, 64, 10, 0, "none"), ("wide", 257, 1, 3, 2, "mixed"),
         ("wide", 1030, 5, 10, 2 ** 31 - 400, "none"), ("unit", 63, 64, 10, 9, "empty")]
SEED, DRAW = 20260117, 41
