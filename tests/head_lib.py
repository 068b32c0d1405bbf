"""What the tests of the policy's action head share (include/gmpe.h gmpe_head_forward / gmpe_head_backward / gmpe_act_head, gmpe.action_logits /
gmpe.act_head): the fixture of tests/golden/make_heads_fixture.py, the seeded inputs, the case lists, the float64 truth

    logits = features @ W.T + b;   grad_features = g @ W;   grad_weight = g.T @ features;   grad_bias = g.sum(0)

and the restated workspace geometry. err(a) = max|a - a64| / max(1, max|a64|); the device is held to err_dev <= 4 * err_ref + 2^-23 per array, err_ref
being the error of the same formulas in float32 torch on the CPU, capped at 1e-5 (tests/test_head_host.py asserts the cap for every case)."""
import functools
import os
import types

import numpy as np
import torch

H = 64
TILE = 256                      # rows per workgroup of the row kernels (gmpe_ppo_rows.h TILE)
MAX_PARTS, PART_ROWS = 128, 32  # gmpe_wgrad.h
CAP = 1e-5
FLOOR = 2.0 ** -23
KS = (1, 5, 24, 25, 64)         # S = K and S = K + 1, the smallest, the largest, the shipped one
ROWS = (1, 65, 255, 256, 257, 513, 4097)        # a lone row, a wave edge, a tile edge, several tiles, partition at its cap with part_rows = 33
SOURCES = ("random", "actor", "rotate")         # weights: randn / 8, and the two shipped heads (K = 25)
CASES = tuple((rows, K, "random") for K in KS for rows in ROWS) + tuple((rows, 25, s) for s in SOURCES[1:] for rows in (257, 4097))
ARRAYS = ("logits", "grad_features", "grad_weight", "grad_bias")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "policy_heads.npz")


def case_id(case):
    return "rows%d-K%d-%s" % case


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as d:
        return {k: d[k] for k in d.files}


def partition(rows):
    """gmpe_wgrad.h partition(rows) -> (nparts, part_rows)"""
    nparts = min(MAX_PARTS, (rows + PART_ROWS - 1) // PART_ROWS)
    return nparts, (rows + nparts - 1) // nparts


def workspace_bytes(rows):
    """the restated layout of gmpe_head_workspace_bytes: f64 [nparts][64][64], then f64 [ceil(rows / 256)][64]"""
    return partition(rows)[0] * H * H * 8 + ((rows + TILE - 1) // TILE) * H * 8


def weights(K, source="random"):
    """(weight [K, 64], bias [K]) float32: randn / 8 and 0.1 randn, or a shipped head"""
    if source == "random":
        rng = np.random.RandomState(500 + K)
        return (rng.randn(K, H) / 8).astype(np.float32), (0.1 * rng.randn(K)).astype(np.float32)
    g = golden()
    w, b = g[source + ".act.action_out.linear.weight"], g[source + ".act.action_out.linear.bias"]
    assert w.shape == (K, H) and b.shape == (K,)
    return w, b


def inputs(rows, K, seed=0):
    """features ~ N(0, 1) [rows, 64] (what a LayerNorm hands over), grad_logits ~ N(0, 1) [rows, K]; float32"""
    rng = np.random.RandomState(7000 + 131 * K + rows + 7919 * seed)
    return rng.randn(rows, H).astype(np.float32), rng.randn(rows, K).astype(np.float32)


def formulas(f, w, b, g, dtype):
    """the four arrays in torch on the CPU in `dtype` -> {name: float64 array}"""
    f, w, b, g = (torch.from_numpy(np.asarray(a)).to(dtype) for a in (f, w, b, g))
    res = dict(logits=f @ w.t() + b, grad_features=g @ w, grad_weight=g.t() @ f, grad_bias=g.sum(0))
    return {k: v.double().numpy() for k, v in res.items()}


def err(a, a64):
    a, a64 = np.asarray(a, np.float64).reshape(-1), np.asarray(a64, np.float64).reshape(-1)
    assert a.shape == a64.shape
    return float(np.abs(a - a64).max() / max(1.0, np.abs(a64).max()))


def bound(err_ref):
    return 4.0 * err_ref + FLOOR


def truth_of(f, w, b, g):
    """(float64 truth, err_ref per array) of one set of inputs"""
    t64 = formulas(f, w, b, g, torch.float64)
    r32 = formulas(f, w, b, g, torch.float32)
    return t64, {k: err(r32[k], t64[k]) for k in t64}


@functools.lru_cache(maxsize=None)
def truth(case):
    """(features, weight, bias, grad_logits, float64 truth, err_ref) of a case; computed once, shared, never written to"""
    rows, K, source = case
    w, b = weights(K, source)
    f, g = inputs(rows, K)
    return (f, w, b, g) + truth_of(f, w, b, g)


def act_layer(K=25, source="random", device="cpu"):
    """a stand-in with the reference's ACTLayer attribute names: .action_out.linear, .multi_discrete, .mixed_action"""
    w, b = weights(K, source)
    lin = torch.nn.Linear(H, K)
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(w))
        lin.bias.copy_(torch.from_numpy(b))
    act = torch.nn.Module()
    act.multi_discrete, act.mixed_action = False, False
    act.action_out = torch.nn.Module()
    act.action_out.linear = lin
    return act.to(device)


class PopArt(object):
    """The tensors of the reference's PopArt(64, 1) from the shipped critic's v_out, weight and bias as Parameters (popart.py:30-41), fresh statistics"""

    def __init__(self, device="cpu"):
        g = golden()
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self.beta, self.epsilon, self.norm_axes, self.output_shape = 0.99999, 1e-5, 1, 1
        self.weight, self.bias = torch.nn.Parameter(t(g["critic.v_out.weight"])), torch.nn.Parameter(t(g["critic.v_out.bias"]))
        self.stddev = t(g["critic.v_out.stddev"])
        self.mean, self.mean_sq = torch.zeros(1, device=device), torch.zeros(1, device=device)
        self.debiasing_term = torch.zeros((), device=device)


def namespace(**kw):
    return types.SimpleNamespace(**kw)
