"""Shared by tests/golden/make_popart_fixture.py, tests/test_popart_host.py and tests/test_gpu_popart_loss.py: input families for the PPO loss with PopArt
(include/gmpe.h gmpe_ppo_loss_popart, gmpe.ppo_losses_popart) and the restatement of the reference lines in torch-CPU — float64 (the yardstick) and float32
(the reference's own ops in the reference's order, the alias of old_mean included).

Restated lines: values = F.linear(critic_features, W, b) inside evaluate_actions, BEFORE the update (graph_mappo.py:160-172, popart.py:55-60);
cal_value_loss (graph_mappo.py:89-117) with PopArt.update then normalize (popart.py:62-99). The policy side is ppo_loss_lib.restate, unchanged.

`restate(..., values=v)` evaluates everything downstream of the value head AT the given values (the device's own): the head's summation order is the
device's choice, so its values are checked on their own with the dot-product bound (H + 2) * U * (sum_j |F_rj * W_j| + |b|), which holds for any order,
and everything after them with the tolerances of ppo_loss_lib (C_DEV * U * (1 + |x|), gradients multiplied back by their denominator).

Constants of this file:
    C_ROW  = ppo_loss_lib.C_DEV  grad_features: per element, in units of U * (1 + |D * g_r * W_j|). Measured float32-restatement-vs-float64 error of
             D * grad_features on the committed families: 10.0 units (tests/test_popart_host.py re-derives it and asserts 4 * measured <= C_DEV), so no new
             constant is needed: the existing C_DEV = 160 covers it.
    C_LAYER = 8   weight_out / bias_out against the float64 rescale fed the SAME statistics: five float32 roundings (s*b, +m, -m, /s'; W*s, /s') and the
             cancellation (s*b + m) - m, whose error is U * |m| <= U * (1 + |x|)-sized only while |m| stays of the order of |s*b|; the bias bound therefore
             carries |mean| / stddev' explicitly (layer_bounds).
"""
import numpy as np
import torch

import ppo_loss_lib as P

U = P.U
C_ROW = P.C_DEV
C_LAYER = 8.0
VARIANTS = ("post_update_values", "true_old_mean", "debiased_stddev", "masked_stats", "raw_normalize")
STATE = ("weight", "bias", "stddev", "mean", "mean_sq", "debiasing_term")
BETA, EPSILON = 0.99999, 1e-5


def cfg(**kw):
    """ppo_loss_lib.cfg with use_popart set (and use_valuenorm clear, as the reference asserts)."""
    return P.cfg(**kw)._replace(use_popart=True, use_valuenorm=False)


def fresh_popart(H, seed=0, exact=False):
    """PopArt(H, 1) after reset_parameters (popart.py:45-53) as float32 arrays; exact: weights multiples of 1/8 in [-1, 1], the bias a multiple of 1/8."""
    rng = np.random.RandomState(1000 + seed * 13 + H)
    if exact:
        w = rng.randint(-8, 9, (1, H)) / 8.0
        w[0, 0] = 0.5 if w[0, 0] == 0 else w[0, 0]
        b = np.array([rng.randint(-8, 9) / 8.0])
    else:
        bound = 1.0 / np.sqrt(H)
        w = rng.uniform(-bound, bound, (1, H))
        w[0, 0] = np.sign(w[0, 0] + 1e-30) * max(abs(w[0, 0]), 0.5 * bound)          # column 0 carries the row's target value (features)
        b = rng.uniform(-bound, bound, (1,))
    f32 = np.float32
    return dict(weight=w.astype(f32), bias=b.astype(f32), stddev=np.ones(1, f32), mean=np.zeros(1, f32), mean_sq=np.zeros(1, f32),
                debiasing_term=np.zeros((), f32))


def vn_state(st):
    """The statistics of a PopArt as the ValueNorm state ppo_loss_lib.family separates its decisions under (the two normalise alike: debiased)."""
    return dict(running_mean=st["mean"], running_mean_sq=st["mean_sq"], debiasing_term=st["debiasing_term"])


def features(values, st, H, seed=0):
    """float32 [B, H] critic features whose value head output is `values` up to the rounding of column 0."""
    B = len(values)
    rng = np.random.RandomState(77 + seed * 31 + B * 7 + H)
    F = rng.randn(B, H)
    W, b = st["weight"].astype(np.float64).reshape(-1), float(st["bias"].reshape(-1)[0])
    F[:, 0] += (np.asarray(values, np.float64).reshape(-1) - (F @ W + b)) / W[0]
    return F.astype(np.float32)


def family(B, K, H, st, c, seed=0, masks="mixed", avail="given", actions="f32"):
    """The generic family of ppo_loss_lib with the values replaced by critic features that produce them under the layer `st`."""
    inp = P.family("generic", B, K, seed=seed, c=c._replace(use_valuenorm=True, use_popart=False), state=vn_state(st), masks=masks, avail=avail,
                   actions=actions)
    inp["features"] = features(inp["values"], st, H, seed)
    return inp


def exact_inputs(B, K, H, c, seed=0):
    """Returns multiples of 1/8 in [-16, 16], features multiples of 1/4 in [-2, 2]: with fresh_popart(exact=True) every row sum and every dot product
    of the FIRST minibatch is exact in float32 in any order. (After it the weights are (W * s) / s', no longer short, so later dot products round.)"""
    inp = P.family("generic", B, K, seed=seed, c=c._replace(use_valuenorm=False, use_popart=False), masks="mixed")
    rng = np.random.RandomState(4242 + seed)
    inp["returns"] = (rng.randint(-128, 129, (B, 1)) / 8.0).astype(np.float32)
    inp["features"] = (rng.randint(-8, 9, (B, H)) / 4.0).astype(np.float32)
    inp["value_preds"] = (rng.randint(-64, 65, (B, 1)) / 16.0).astype(np.float32)
    return inp


def _sqrt(x):
    """sqrt through NumPy: correctly rounded on every CPU. torch's CPU sqrt goes through a vector maths library whose float32 result may differ in the
    last bit from one CPU to another, which a restatement that is compared bit for bit cannot afford; every other op used here is a basic IEEE one."""
    return torch.from_numpy(np.sqrt(x.detach().numpy()))


def rescale_layer(weight, bias, s_old, mean_new, mean_sq_new, dtype=torch.float64):
    """Steps 4-6 of PopArt.update given the updated raw statistics: (stddev', W', b') with the aliased old_mean."""
    t = lambda a: torch.tensor(np.asarray(a, np.float32)).to(dtype)
    W, b, s, m, q = t(weight), t(bias), t(s_old), t(mean_new), t(mean_sq_new)
    s_new = _sqrt(q - m ** 2).clamp(min=1e-4)
    return s_new.numpy(), (W * s / s_new).numpy(), ((s * b + m - m) / s_new).numpy()


def layer_bounds(weight, bias, s_old, mean_new, s_new):
    """C_LAYER * U * (1 + |x|) for W'; for b' the cancellation (s*b + m) - m adds its operands' rounding: U * (|s*b| + 2|m|) / s'."""
    f = lambda a: np.abs(np.asarray(a, np.float64))
    w = C_LAYER * U * (1.0 + f(weight) * f(s_old) / f(s_new))
    b = C_LAYER * U * (1.0 + (f(s_old) * f(bias) + 2.0 * f(mean_new)) / f(s_new))
    return w, b


def restate(inp, c, st, dtype=torch.float64, beta=BETA, epsilon=EPSILON, variant=None, values=None):
    """The reference lines in `dtype` on the CPU. inp: ppo_loss_lib's arrays with `features` [B, H] in place of `values`; st: the six PopArt arrays
    (read; the updated ones are returned under "state"). values: evaluate everything after the head at these values instead of the head's own.
    variant: one of VARIANTS, a cheap wrong version."""
    assert variant is None or variant in VARIANTS
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float32)).to(dtype)
    F = t(inp["features"])
    B, H = F.shape
    W, b, s_old = t(st["weight"]).reshape(1, H), t(st["bias"]).reshape(1), t(st["stddev"]).reshape(1)
    mean, msq, db = t(st["mean"]).reshape(1).clone(), t(st["mean_sq"]).reshape(1).clone(), t(st["debiasing_term"]).reshape(()).clone()
    vp, ret, am = (t(inp[k]).reshape(-1, 1) for k in ("value_preds", "returns", "active_masks"))
    head = torch.nn.functional.linear(F, W, b)                              # evaluate_actions runs first: the pre-update weights
    # ---- PopArt.update (popart.py:62-83)
    old_mean_copy = mean.clone()
    old_mean = mean                                                        # the alias: old_mean IS self.mean
    rows = ret[am.reshape(-1) != 0] if variant == "masked_stats" else ret
    bm, bsq = rows.mean(dim=0), (rows ** 2).mean(dim=0)
    mean.mul_(beta).add_(bm * (1.0 - beta))
    msq.mul_(beta).add_(bsq * (1.0 - beta))
    db.mul_(beta).add_(1.0 * (1.0 - beta))
    dcl = db.clamp(min=epsilon)
    mean_d = mean / dcl
    var_raw_d = msq / dcl - mean_d ** 2
    s_new = _sqrt(var_raw_d if variant == "debiased_stddev" else (msq - mean ** 2)).clamp(min=1e-4)
    W_new = W * s_old / s_new
    b_new = (s_old * b + (old_mean_copy if variant == "true_old_mean" else old_mean) - mean) / s_new
    if variant == "post_update_values":
        head = torch.nn.functional.linear(F, W_new, b_new)
    v = (head if values is None else t(values).reshape(B, 1)).detach().clone().requires_grad_(True)
    # ---- normalize (popart.py:85-99)
    if variant == "raw_normalize":
        R = (ret - mean[None]) / s_new[None]
    else:
        R = (ret - mean_d[None]) / _sqrt(var_raw_d.clamp(min=1e-2))[None]
    # ---- cal_value_loss (graph_mappo.py:89-117), as ppo_loss_lib.restate
    d = v - vp
    vpc = vp + d.clamp(-c.clip_param, c.clip_param)
    e_c, e_o = R - vpc, R - v

    def huber(e, dl):
        a = (abs(e) <= dl).to(dtype)
        bb = (e > dl).to(dtype)                                             # util.py:26: b = (e > d)
        return a * e ** 2 / 2 + bb * dl * (abs(e) - dl / 2)
    if c.use_huber_loss:
        L_c, L_o = huber(e_c, c.huber_delta), huber(e_o, c.huber_delta)
    else:
        L_c, L_o = e_c ** 2 / 2, e_o ** 2 / 2
    L = torch.max(L_o, L_c) if c.use_clipped_value_loss else L_o
    vm = c.use_value_active_masks
    value_loss = (L * am).sum() / am.sum() if vm else L.mean()
    value_loss.backward()
    g = v.grad                                                              # d value_loss / d values [B, 1]
    n = lambda x: x.detach().numpy().copy()
    Dv = float(am.sum()) if vm else float(B)
    wv = n(am) if vm else np.ones((B, 1))
    pol = P.restate(dict(inp, values=np.zeros((B, 1), np.float32)), c._replace(use_valuenorm=False, use_popart=False), dtype)     # the policy side
    out = {k: pol[k] for k in ("policy_loss", "dist_entropy", "actor_loss", "ratio_mean", "denom_policy", "action_log_probs", "imp_weights", "grad_logits",
                               "abs_policy", "abs_entropy", "abs_ratio")}
    gF = g * W                                                              # addmm's backward: one product per element, through the pre-update weights
    out.update(values=n(head), value_loss=n(value_loss), denom_value=Dv, grad_values=n(g), grad_features=n(gF), grad_weight=n((g * F).sum(0, keepdim=True)),
               grad_bias=n(g.sum().reshape(1)), abs_value=float(np.abs(n(L) * wv).sum()), abs_grad_weight=n((g * F).abs().sum(0, keepdim=True)),
               abs_grad_bias=float(n(g.abs().sum())), abs_head=n((F * W).abs().sum(1, keepdim=True) + b.abs()),
               state=dict(weight=n(W_new), bias=n(b_new), stddev=n(s_new), mean=n(mean), mean_sq=n(msq), debiasing_term=n(db)))
    return out


def value_bound(ref):
    """(H + 2) * U * (sum_j |F_rj * W_j| + |b|) per row: the float32 dot product in any order, plus the bias add."""
    H = ref["grad_features"].shape[1]
    return (H + 2) * U * ref["abs_head"]


def sum_bound(B, abs_terms):
    """(log2(B) + 4) * U * sum|terms|: a sum of B inexact float32 terms, however it is ordered (and exactly rounded once at the end on the device)."""
    return (np.log2(max(B, 2)) + 4) * U * np.asarray(abs_terms, np.float64)


def stat_tol(inp, k):
    """The ValueNorm-state bound of tests/test_gpu_ppo_loss.py: float32 summation noise of the batch means."""
    B = len(inp["returns"])
    x = inp["returns"].astype(np.float64)
    if k == "debiasing_term":
        return 2 * U
    return (np.log2(max(B, 2)) + 4) * U * float(np.abs(x ** 2 if k == "mean_sq" else x).mean())


def head_error(r32, r64):
    """The largest error of float32 D * grad_features against float64 (both evaluated at the same values), in units of U * (1 + |x|)."""
    D = r64["denom_value"]
    return float(P.row_err(r32["grad_features"] * D, r64["grad_features"] * D).max())


# (B, K, H, cfg keywords, masks): the families C_ROW is checked on and the GPU suite's generic cases
CASES = [(96, 25, 8, dict(), "mixed"), (96, 5, 64, dict(pm=False, vm=False, clipped=False, huber=False), "mixed"), (257, 9, 65, dict(huber_delta=0.5), "ones")]
SHAPE_ROWS, SHAPE_H = (1, 63, 256, 257, 700), (1, 3, 4, 64, 65, 256)
