"""Shared by tests/test_ppo_loss_host.py and tests/test_gpu_ppo_loss.py: input families for the PPO loss arithmetic (gmpe_ppo_loss), and the restatement
of the reference lines in torch-CPU — float64 (the yardstick) and float32 (the reference's own arithmetic: the same torch ops in the same order).

Restated lines: Categorical.forward + ACTLayer.evaluate_actions (onpolicy/algorithms/utils/distributions.py:84-91, act.py:212-220), the ratio / clip /
surrogate block of GR_MAPPO.ppo_update (onpolicy/algorithms/graph_mappo.py:176-207), cal_value_loss (:89-117) with ValueNorm.update / normalize
(onpolicy/utils/valuenorm.py:48-85) and huber_loss / mse_loss (onpolicy/utils/util.py:24-30). Gradients come from torch's autograd on those ops, as in
the reference. tests/test_ppo_loss_host.py pins both restatements to tests/golden/ppo_loss.npz (the reference's own run).

Tolerances: per element c * U * (1 + |x|), U = 2**-24, x the float64 value; gradients are compared after multiplying back by the
denominator. c is four times the largest error of the float32 restatement against the float64 one over the families below, in the same units:
    C_REF  = 40   measured 34.7 on the families of ALL_CASES (tests/test_ppo_loss_host.py re-derives it and asserts it stays below C_REF)
    C_DEV  = 160  = 4 * C_REF: device exp / log may each differ from glibc's by an ulp or two, and K + 1 of them enter a row
"""
import collections

import numpy as np
import torch

U = 2.0 ** -24
C_REF = 40.0          # measured 34.7 (float32 torch-CPU restatement vs float64, units of U * (1 + |x|)); rounded up
C_DEV = 4.0 * C_REF   # what the device gets
FMIN32 = float(torch.finfo(torch.float32).min)
MARGIN = 1e-4         # every decision is an exact tie or separated by this relative margin (test_ppo_loss_host.py (b))

Cfg = collections.namedtuple("Cfg", ["clip_param", "huber_delta", "entropy_coef", "use_policy_active_masks", "use_value_active_masks",
                                     "use_clipped_value_loss", "use_huber_loss", "use_valuenorm", "use_popart"])
VARIANTS = ("symmetric_huber", "plain_means", "stale_stats", "unmasked_logits", "masked_leak", "clamp_leak", "first_max")
COLS = ("value_preds", "returns", "active_masks", "old_action_log_probs", "adv_targ")


def cfg(clip_param=0.25, huber_delta=10.0, entropy_coef=0.01, pm=True, vm=True, clipped=True, huber=True, valuenorm=False):
    # clip 0.25: 1 - clip, 1 + clip and clip are exact in float32 and float64 alike, so "exactly at the bound" means the same in both
    return Cfg(clip_param, huber_delta, entropy_coef, pm, vm, clipped, huber, valuenorm, False)


def fresh_state():
    """ValueNorm(1) after reset_parameters (valuenorm.py:34-46)."""
    return dict(running_mean=np.zeros(1, np.float32), running_mean_sq=np.zeros(1, np.float32), debiasing_term=np.zeros((), np.float32))


def restate(inp, c, dtype=torch.float64, state=None, beta=0.99999, epsilon=1e-5, variant=None):
    """The reference lines in `dtype` on the CPU. inp: float32 NumPy arrays logits [B, K], values, actions, COLS [B, 1], available_actions [B, K] or None.
    state: ValueNorm's three arrays (read; the updated ones are returned). variant: one of VARIANTS, a cheap wrong version (host test (c))."""
    assert variant is None or variant in VARIANTS
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float32)).to(dtype)
    logits, values = t(inp["logits"]).requires_grad_(True), t(inp["values"]).requires_grad_(True)
    act = torch.tensor(np.asarray(inp["actions"])).long().reshape(-1, 1)
    vp, ret, am, old, adv = (t(inp[k]).reshape(-1, 1) for k in COLS)
    avail = None if inp.get("available_actions") is None else t(inp["available_actions"])
    B = logits.shape[0]
    # ---- Categorical.forward (distributions.py:84-91): masked entries at finfo(float32).min in either precision (what the device holds)
    x = logits.clone()
    if avail is not None and variant != "unmasked_logits":
        if variant == "masked_leak":
            x = torch.where(avail == 0, logits + (FMIN32 - logits).detach(), logits)
        else:
            x[avail == 0] = FMIN32
    # FixedCategorical(logits=x) is torch.distributions.Categorical: logits - logsumexp at construction, probs = softmax of that (lazily, at entropy()),
    # entropy = -(clamp(logits, finfo.min) * probs).sum(-1). Called in evaluate_actions' order (log-probs, then entropy): autograd adds the three
    # gradient paths into the logits in the order their nodes were made, which is part of the float32 result.
    dist = torch.distributions.Categorical(logits=x)
    l = dist.logits
    logp = dist.log_prob(act.squeeze(-1)).view(B, -1).sum(-1).unsqueeze(-1)        # FixedCategorical.log_probs (distributions.py:18-25)
    ent_row = dist.entropy()
    pm = c.use_policy_active_masks and variant != "plain_means"
    vm = c.use_value_active_masks and variant != "plain_means"
    dist_entropy = (ent_row * am.squeeze(-1)).sum() / am.sum() if pm else ent_row.mean()      # act.py:215-220
    # ---- graph_mappo.py:176-197
    ratio = torch.exp(logp - old)
    surr1 = ratio * adv
    rc = torch.clamp(ratio, 1.0 - c.clip_param, 1.0 + c.clip_param)
    if variant == "clamp_leak":
        rc = ratio + (rc - ratio).detach()
    surr2 = rc * adv
    mn = torch.sum(torch.min(surr1, surr2), dim=-1, keepdim=True)
    policy_loss = (-mn * am).sum() / am.sum() if pm else -mn.mean()
    actor_loss = policy_loss - dist_entropy * c.entropy_coef
    actor_loss.backward()
    # ---- cal_value_loss (graph_mappo.py:89-117)
    d = values - vp
    dc = d.clamp(-c.clip_param, c.clip_param)
    if variant == "clamp_leak":
        dc = d + (dc - d).detach()
    vpc = vp + dc
    new_state = None
    R = ret
    if c.use_valuenorm:
        rm, rms, db = (t(state[k]) for k in ("running_mean", "running_mean_sq", "debiasing_term"))

        def mean_std():
            mean, msq = rm / db.clamp(min=epsilon), rms / db.clamp(min=epsilon)
            return mean, torch.sqrt((msq - mean ** 2).clamp(min=1e-2))
        stale = mean_std()
        with torch.no_grad():                                       # ValueNorm.update (valuenorm.py:56-73)
            bm, bsq = ret.mean(dim=0), (ret ** 2).mean(dim=0)
            rm = rm * beta + bm * (1.0 - beta)
            rms = rms * beta + bsq * (1.0 - beta)
            db = db * beta + 1.0 * (1.0 - beta)
        mean, std = stale if variant == "stale_stats" else mean_std()
        R = (ret - mean[None]) / std[None]                          # normalize (:75-85)
        new_state = dict(running_mean=rm.numpy().copy(), running_mean_sq=rms.numpy().copy(), debiasing_term=db.numpy().copy())
    e_c, e_o = R - vpc, R - values

    def huber(e, dl):
        a = (abs(e) <= dl).to(dtype)
        b = ((abs(e) > dl) if variant == "symmetric_huber" else (e > dl)).to(dtype)     # util.py:26: b = (e > d)
        return a * e ** 2 / 2 + b * dl * (abs(e) - dl / 2)
    if c.use_huber_loss:
        L_c, L_o = huber(e_c, c.huber_delta), huber(e_o, c.huber_delta)
    else:
        L_c, L_o = e_c ** 2 / 2, e_o ** 2 / 2
    if c.use_clipped_value_loss:
        L = torch.where(L_o >= L_c, L_o, L_c) if variant == "first_max" else torch.max(L_o, L_c)
    else:
        L = L_o
    value_loss = (L * am).sum() / am.sum() if vm else L.mean()
    value_loss.backward()
    n = lambda v: v.detach().numpy()
    Dp = float(am.sum()) if pm else float(B)
    Dv = float(am.sum()) if vm else float(B)
    wp = n(am) if pm else np.ones((B, 1))
    wv = n(am) if vm else np.ones((B, 1))
    out = dict(policy_loss=n(policy_loss), dist_entropy=n(dist_entropy), actor_loss=n(actor_loss), value_loss=n(value_loss), ratio_mean=n(ratio.mean()),
               denom_policy=Dp, denom_value=Dv, action_log_probs=n(logp), imp_weights=n(ratio), entropy_rows=n(ent_row), value_rows=n(L),
               grad_logits=n(logits.grad), grad_values=n(values.grad), state=new_state,
               # sums of |term| for the scalar bounds ((c + 2) * U * sum|term| / denominator)
               abs_policy=float(np.abs(n(mn) * wp).sum()), abs_entropy=float(np.abs(n(ent_row)[:, None] * wp).sum()),
               abs_value=float(np.abs(n(L) * wv).sum()), abs_ratio=float(np.abs(n(ratio)).sum()),
               decisions=dict(ratio=n(ratio), lo=1.0 - c.clip_param, hi=1.0 + c.clip_param, surr1=n(surr1), surr2=n(surr2), e_o=n(e_o), e_c=n(e_c),
                              L_o=n(L_o), L_c=n(L_c), d=n(d), clip=c.clip_param, delta=c.huber_delta))
    return out


def rel_gap(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    den = np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300)
    return np.abs(a - b) / den


def decision_gaps(dec, c):
    """name -> relative gap per row of every comparison the arithmetic branches on (0: an exact tie)."""
    g = dict(ratio_lo=rel_gap(dec["ratio"], dec["lo"]), ratio_hi=rel_gap(dec["ratio"], dec["hi"]), surr=rel_gap(dec["surr1"], dec["surr2"]),
             d_hi=rel_gap(dec["d"], dec["clip"]), d_lo=rel_gap(dec["d"], -dec["clip"]))
    if c.use_huber_loss:
        for k in ("e_o", "e_c"):
            g["abs_" + k] = rel_gap(np.abs(dec[k]), dec["delta"])
            g[k] = rel_gap(dec[k], dec["delta"])
    if c.use_clipped_value_loss:
        g["branches"] = rel_gap(dec["L_o"], dec["L_c"])
    return g


def undecided(inp, c, state=None):
    """Rows with a decision that is neither an exact tie nor separated by MARGIN, on the float64 restatement."""
    gaps = decision_gaps(restate(inp, c, torch.float64, state)["decisions"], c)
    bad = np.zeros(len(inp["logits"]), bool)
    for v in gaps.values():
        v = v.reshape(len(bad), -1).max(axis=1) if v.ndim > 1 else v
        bad |= (v.reshape(-1) > 0) & (v.reshape(-1) < MARGIN)
    return bad


def _q(a, step=1.0 / 1024):
    """Multiples of 2**-10: v, value_preds and their sums / differences are exact in float32, so vp + (v - vp) == v inside the clip range (an exact branch tie)."""
    return (np.round(np.asarray(a, np.float64) / step) * step).astype(np.float32)


def _draw(rng, B, K, family, clip):
    f32 = np.float32
    logits = (rng.randn(B, K) * 2.0).astype(f32)
    actions = rng.randint(0, K, (B, 1))
    avail = (rng.rand(B, K) < 0.7).astype(f32)
    avail[np.arange(B), actions[:, 0]] = 1.0
    adv = rng.randn(B, 1).astype(f32)
    dlog = rng.choice([0.05, 0.5, -0.5, -0.05, 0.9, -0.9], size=(B, 1)) * (0.5 + rng.rand(B, 1))   # ratios inside the range, above and below it
    vp = _q(rng.randn(B, 1) * 2)
    dv = rng.choice([0.1, -0.1, 0.6, -0.6], size=(B, 1)) * (0.3 + rng.rand(B, 1))                 # value deltas inside and outside the clip
    v = _q(vp + dv)
    err = rng.choice([0.3, -0.3, 3.0, -3.0, 14.0, -14.0], size=(B, 1)) * (0.5 + rng.rand(B, 1))   # errors inside a small delta, beyond 10, below -10
    ret = (v + err).astype(f32)
    if family == "edges":
        logits = (rng.rand(B, K) * 60 - 30).astype(f32)                                          # +-30: the max subtraction matters
        k = np.arange(B) % 5
        avail[k == 0] = 1.0                                                                       # all available
        stop = k == 1                                                                             # stop rows: one available action
        avail[stop] = 0.0
        avail[stop, actions[stop, 0]] = 1.0
        actions[k == 2] = 0                                                                       # first and last column
        actions[k == 3] = K - 1
        avail[np.arange(B), actions[:, 0]] = 1.0
        allm = k == 4                                                                             # nothing available: the reference gives a uniform row, no gradient
        avail[allm] = 0.0
        adv[np.arange(B) % 7 == 0] = 0.0
        adv[np.arange(B) % 7 == 1] = -0.0
    if family == "ties":
        k = np.arange(B) % 4
        v[k == 0] = vp[k == 0] + f32(clip)                                                        # value delta exactly at +clip / -clip
        v[k == 1] = vp[k == 1] - f32(clip)
        mirror = k == 2                                                                           # mse mirror: R - v == -(R - vpc), the branch losses tie exactly
        v[mirror] = vp[mirror] + f32(0.75)
        ret = ret.copy()
        ret[mirror] = vp[mirror] + f32(0.5 * (0.75 + clip))
        ret[~mirror] = _q(ret[~mirror])
    inp = dict(logits=logits, values=v, actions=actions.astype(f32), available_actions=avail, value_preds=vp, returns=ret,
               active_masks=np.ones((B, 1), f32), adv_targ=adv)
    # old log-probs: the float64 log-prob of the action plus the drawn offset
    z = dict(inp, old_action_log_probs=np.zeros((B, 1), f32))
    lp = restate(z, cfg(clip_param=clip))["action_log_probs"]
    old = (lp - dlog).astype(f32)
    if family in ("edges", "ties"):
        one = avail.sum(1) == 1                                                                   # stop rows: log-prob exactly 0, ratio exactly 1
        old[one] = 0.0
    inp["old_action_log_probs"] = old
    return inp


def family(name, B, K, seed=0, c=None, state=None, masks="ones", avail="given", actions="f32"):
    """Inputs of one family. Rows whose decisions are neither exact ties nor separated by MARGIN under `c` (with `state`) are redrawn: a condition on the
    inputs, so no row is ever left out of a comparison. masks: ones | mixed | single | zero; avail: given | none | ones."""
    c = c or cfg()
    rng = np.random.RandomState(seed * 7919 + B * 31 + K)
    inp = _draw(rng, B, K, name, c.clip_param)

    def finish(inp):
        out = dict(inp)
        m = np.ones((B, 1), np.float32)
        if masks == "mixed":
            m = (np.arange(B) % 3 != 1).astype(np.float32).reshape(B, 1)
        elif masks == "single":
            m[:] = 0.0
            m[B // 2] = 1.0
        elif masks == "zero":
            m[:] = 0.0
        out["active_masks"] = m
        if avail == "none":
            out["available_actions"] = None
        elif avail == "ones":
            out["available_actions"] = np.ones((B, K), np.float32)
        if actions == "int64":
            out["actions"] = out["actions"].astype(np.int64)
        return out
    for _ in range(40):
        cur = finish(inp)
        bad = undecided(cur, c, state) if masks != "zero" else np.zeros(B, bool)
        if not bad.any():
            return cur
        new = _draw(rng, B, K, name, c.clip_param)
        for k, a in inp.items():
            # a redrawn row keeps its place in the family's pattern (the patterns are functions of the row index)
            a[bad] = new[k][bad]
    raise AssertionError("could not separate the decisions of family %s" % name)


def row_err(got, want):
    """|got - want| in units of U * (1 + |want|)."""
    want = np.asarray(want, np.float64)
    return np.abs(np.asarray(got, np.float64) - want) / (U * (1.0 + np.abs(want)))


def scalar_bounds(ref, cc):
    """(c + 2) * U * sum|term| / denominator for the four scalars; actor_loss adds its two parts."""
    k = (cc + 2.0) * U
    b = dict(policy_loss=k * ref["abs_policy"] / ref["denom_policy"], dist_entropy=k * ref["abs_entropy"] / ref["denom_policy"],
             value_loss=k * ref["abs_value"] / ref["denom_value"], ratio_mean=k * ref["abs_ratio"] / len(ref["imp_weights"]))
    return b


# the cases over which C_REF is measured and which the GPU suite runs (family, B, K, cfg keywords, masks, avail)
ALL_CASES = [("generic", 257, 25, dict(), "mixed", "given"), ("generic", 300, 5, dict(huber_delta=0.5), "ones", "given"),
             ("generic", 257, 25, dict(valuenorm=True), "mixed", "given"), ("generic", 64, 64, dict(huber=False), "mixed", "none"),
             ("edges", 260, 25, dict(), "mixed", "given"), ("edges", 130, 8, dict(huber_delta=0.5, clipped=False), "ones", "given"),
             ("edges", 65, 1, dict(), "ones", "ones"), ("edges", 63, 2, dict(), "single", "given"),
             ("ties", 256, 9, dict(huber=False), "mixed", "given"), ("ties", 255, 24, dict(), "ones", "given"),
             ("generic", 1000, 33, dict(pm=False, vm=False), "mixed", "given"),
             # clip_param 0: 1 - clip == 1 + clip == 1, so the stop rows (log-prob exactly 0, old log-prob 0, ratio exactly 1) sit exactly on BOTH clip
             # bounds, in float32 and float64 alike; with K = 1 every row does
             ("edges", 260, 25, dict(clip_param=0.0), "mixed", "given"), ("edges", 65, 1, dict(clip_param=0.0, huber=False), "ones", "given")]
RATIO_TIE_CASES = [c for c in ALL_CASES if c[3].get("clip_param") == 0.0]


def case_inputs(case, seed=0):
    name, B, K, kw, masks, avail = case
    c = cfg(**kw)
    st = fresh_state() if c.use_valuenorm else None
    return family(name, B, K, seed=seed, c=c, state=st, masks=masks, avail=avail), c, st


def reference_error(ref32, ref64):
    """The largest error of the float32 restatement against the float64 one over the per-row outputs and gradients, in units of U * (1 + |x|)."""
    worst = 0.0
    for k, scale in (("action_log_probs", 1.0), ("imp_weights", 1.0), ("grad_logits", ref64["denom_policy"]), ("grad_values", ref64["denom_value"])):
        worst = max(worst, float(row_err(ref32[k] * scale, ref64[k] * scale).max()))
    return worst
