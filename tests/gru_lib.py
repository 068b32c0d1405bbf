"""What the tests of the masked GRU layer (include/gmpe.h gmpe_gru_forward / gmpe_gru_backward, gmpe.rnn_layer) share: the seeded inputs of
tests/golden/make_gru_fixture.py, and a NumPy float64 restatement of RNNLayer.forward (onpolicy/algorithms/utils/rnn.py:23-79, recurrent_N == 1) in two
forms — per-row masking (what the kernels do) and the reference's segment loop — with its hand-written backward.

err(a) = max|a - a64| / max(1, max|a64|); the device is held to err_dev <= 4 * err_ref + 2^-23 per array, err_ref being the error of the reference's own
float32 run (the fixture), capped at 1e-5."""
import numpy as np

TILE = 32                       # GMPE_GRU_ROW_TILE
H = D = 64
EPS = 1e-5                      # nn.LayerNorm's default
CASES = ((1, 5), (2, 3), (10, 7), (10, 2 * TILE + 1))
PATTERNS = ("ones", "row0_t0", "random", "zeros")
PARAMS = ("weight_ih", "weight_hh", "bias_ih", "bias_hh", "ln_weight", "ln_bias")
GRADS = ("grad_x", "grad_hxs") + tuple("grad_" + k for k in PARAMS)
CAP = 1e-5
FLOOR = 2.0 ** -23


def key(L, Nb, pattern):
    return "L%d_N%d_%s" % (L, Nb, pattern)


def params(seed=0, scale=1.0):
    """weights U(-1/8, 1/8) * scale, biases 0.1 N(0, 1), LayerNorm weight 1 + 0.1 N, bias 0.1 N; float32"""
    rng = np.random.RandomState(1000 + seed)
    f = np.float32
    return dict(weight_ih=(rng.uniform(-0.125, 0.125, (3 * H, D)) * scale).astype(f), weight_hh=(rng.uniform(-0.125, 0.125, (3 * H, H)) * scale).astype(f),
                bias_ih=(0.1 * rng.randn(3 * H)).astype(f), bias_hh=(0.1 * rng.randn(3 * H)).astype(f),
                ln_weight=(1 + 0.1 * rng.randn(H)).astype(f), ln_bias=(0.1 * rng.randn(H)).astype(f))


def inputs(L, Nb, seed=0):
    """x ~ N(0, 1) [L * Nb, D], hxs ~ U(-1, 1) [Nb, 1, H], and the loss weights gf [L * Nb, H], gh [Nb, 1, H] ~ N(0, 1); float32"""
    rng = np.random.RandomState(2000 + 97 * L + Nb + 7919 * seed)
    f = np.float32
    return dict(x=rng.randn(L * Nb, D).astype(f), hxs=rng.uniform(-1, 1, (Nb, 1, H)).astype(f), gf=rng.randn(L * Nb, H).astype(f),
                gh=rng.randn(Nb, 1, H).astype(f))


def masks(L, Nb, pattern, seed=0):
    """[L * Nb, 1] float32 in {0, 1}, time-major"""
    m = np.ones((L, Nb), np.float32)
    if pattern == "row0_t0":
        m[0, 0] = 0
    elif pattern == "random":
        rng = np.random.RandomState(3000 + 31 * L + Nb + seed)
        m[rng.rand(L, Nb) < 0.2] = 0
        m[:, Nb - 1] = 0                                # an all-zero row
        if Nb > 1:
            m[:, 0] = 1
            m[L - 1, 0] = 0                             # a row whose only zero is at the last step
    elif pattern == "zeros":
        m[:] = 0
    elif pattern != "ones":
        raise ValueError(pattern)
    return m.reshape(L * Nb, 1)


def _sig(a):
    return 1.0 / (1.0 + np.exp(-a))


def _step(xt, h, P):
    Wi, Wh, bi, bh = P["weight_ih"], P["weight_hh"], P["bias_ih"], P["bias_hh"]
    gi, gh = xt @ Wi.T + bi, h @ Wh.T + bh
    r, z = _sig(gi[:, :H] + gh[:, :H]), _sig(gi[:, H:2 * H] + gh[:, H:2 * H])
    hn = gh[:, 2 * H:]
    n = np.tanh(gi[:, 2 * H:] + r * hn)
    return (1 - z) * n + z * h, (r, z, n, hn)


def _norm(h, P, eps):
    mean = h.mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(((h - mean) ** 2).mean(-1, keepdims=True) + eps)
    return (h - mean) * rstd * P["ln_weight"] + P["ln_bias"], mean, rstd


def _f64(P):
    return {k: np.asarray(v, np.float64) for k, v in P.items()}


def forward64(x, hxs, m, P, eps=EPS, keep=False):
    """per-row masking: h <- h * masks[t] at every step. -> features [L * Nb, H], hxs_out [Nb, 1, H] (and what backward64 needs)"""
    P = _f64(P)
    Nb = hxs.shape[0]
    L = x.shape[0] // Nb
    x, m = np.asarray(x, np.float64).reshape(L, Nb, -1), np.asarray(m, np.float64).reshape(L, Nb, 1)
    h = np.asarray(hxs, np.float64).reshape(Nb, H)
    hs, saved = [], []
    for t in range(L):
        hp = h * m[t]
        h, gates = _step(x[t], hp, P)
        hs.append(h)
        saved.append((hp,) + gates)
    feats, mean, rstd = _norm(np.stack(hs), P, eps)
    out = feats.reshape(L * Nb, H), h.reshape(Nb, 1, H)
    return out + ((x, m, np.stack(hs), saved, mean, rstd, P),) if keep else out


def segment64(x, hxs, m, P, eps=EPS):
    """the reference's form: the sequence is split at every step t >= 1 at which ANY row has a zero; at a segment's first step every row is multiplied by
    its own mask, inside a segment nothing is."""
    P = _f64(P)
    Nb = hxs.shape[0]
    L = x.shape[0] // Nb
    x, m = np.asarray(x, np.float64).reshape(L, Nb, -1), np.asarray(m, np.float64).reshape(L, Nb, 1)
    h = np.asarray(hxs, np.float64).reshape(Nb, H)
    if L == 1:
        cuts = [0, 1]
    else:
        cuts = [0] + [t for t in range(1, L) if (m[t] == 0).any()] + [L]
    hs = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        h = h * m[a]
        for t in range(a, b):
            h, _ = _step(x[t], h, P)
            hs.append(h)
    feats, _, _ = _norm(np.stack(hs), P, eps)
    return feats.reshape(L * Nb, H), h.reshape(Nb, 1, H)


def backward64(x, hxs, m, P, gf, gh, eps=EPS):
    """the gradients of sum(features * gf) + sum(hxs_out * gh) with per-row masking, float64 -> dict over GRADS"""
    _, _, (x, m, hs, saved, mean, rstd, P) = forward64(x, hxs, m, P, eps, keep=True)
    L, Nb = x.shape[0], x.shape[1]
    gf = np.asarray(gf, np.float64).reshape(L, Nb, H)
    dh = np.asarray(gh, np.float64).reshape(Nb, H).copy()
    Wi, Wh = P["weight_ih"], P["weight_hh"]
    g = {k: np.zeros_like(P[k[5:]]) for k in GRADS[2:]}
    gx = np.zeros_like(x)
    xh = (hs - mean) * rstd
    g["grad_ln_weight"] = (gf * xh).sum((0, 1))
    g["grad_ln_bias"] = gf.sum((0, 1))
    for t in range(L - 1, -1, -1):
        hp, r, z, n, hn = saved[t]
        dxh = gf[t] * P["ln_weight"]
        dt = dh + rstd[t] * (dxh - dxh.mean(-1, keepdims=True) - xh[t] * (dxh * xh[t]).mean(-1, keepdims=True))
        dnp = dt * (1 - z) * (1 - n * n)
        dzp = dt * (hp - n) * z * (1 - z)
        drp = dnp * hn * r * (1 - r)
        dgi, dgh = np.concatenate([drp, dzp, dnp], -1), np.concatenate([drp, dzp, dnp * r], -1)
        gx[t] = dgi @ Wi
        g["grad_weight_ih"] += dgi.T @ x[t]
        g["grad_weight_hh"] += dgh.T @ hp
        g["grad_bias_ih"] += dgi.sum(0)
        g["grad_bias_hh"] += dgh.sum(0)
        dh = (dt * z + dgh @ Wh) * m[t]
    g["grad_x"], g["grad_hxs"] = gx.reshape(L * Nb, -1), dh.reshape(Nb, 1, H)
    return g


def err(a, a64):
    a, a64 = np.asarray(a, np.float64).reshape(-1), np.asarray(a64, np.float64).reshape(-1)
    assert a.shape == a64.shape
    return float(np.abs(a - a64).max() / max(1.0, np.abs(a64).max()))


def bound(err_ref):
    return 4.0 * err_ref + FLOOR


def truth64(L, Nb, pattern, seed=0, scale=1.0):
    """(inputs, masks, params, {array name: float64 value}) of one case"""
    P, I, m = params(seed, scale), inputs(L, Nb, seed), masks(L, Nb, pattern, seed)
    f, ho = forward64(I["x"], I["hxs"], m, P)
    out = dict(features=f, hxs_out=ho)
    out.update(backward64(I["x"], I["hxs"], m, P, I["gf"], I["gh"]))
    return I, m, P, out
