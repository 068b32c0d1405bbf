"""Host side of the PPO loss arithmetic (include/gmpe.h gmpe_ppo_loss, gmpe.ppo_losses), no GPU:
(a) the float32 / float64 restatements of tests/ppo_loss_lib.py reproduce the reference's own run (tests/golden/ppo_loss.npz, made by
    tests/golden/make_ppo_loss_fixture.py: GR_MAPPO.ppo_update on a stub policy, ACTLayer.evaluate_actions, a real ValueNorm over three minibatches);
(b) every decision of every input family is an exact tie or separated by a relative margin of 1e-4;
(c) the inputs tell the truth from cheap wrong variants;
(d) the refusals of the Python layer and of the C entry point, which need no device;
and the error of the reference's own float32 arithmetic, from which the device's tolerance is derived (ppo_loss_lib.C_REF, C_DEV)."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import abi_lib
import gmpe
import ppo_loss_lib as P
from gmpe import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "ppo_loss.npz")
FIX_CASES = ("a", "b", "c", "d", "e")


def fixture_case(d, name):
    """(cfg, K, [(inputs, outputs, state after)] for the three minibatches) of one fixture case."""
    clip, delta, ent = (float(x) for x in d[name + "_cfg"])
    pm, vm, clipped, huber, vnorm = (bool(x) for x in d[name + "_flags"])
    c = P.cfg(clip, delta, ent, pm, vm, clipped, huber, vnorm)
    steps = []
    for i in range(3):
        pre = "%s_%d_" % (name, i)
        inp = {k[len(pre) + 3:]: d[k] for k in d.files if k.startswith(pre + "in_")}
        out = {k[len(pre):]: d[k] for k in d.files if k.startswith(pre) and not k.startswith(pre + "in_") and not k.startswith(pre + "state_")}
        st = {k[len(pre) + 6:]: d[k] for k in d.files if k.startswith(pre + "state_")} or None
        steps.append((inp, out, st))
    return c, int(d[name + "_K"]), steps


def _ulps32(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.maximum(np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64), 1e-45)


# ---------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("name", FIX_CASES)
def test_restatements_reproduce_the_reference_run(name):
    c, K, steps = fixture_case(np.load(GOLD), name)
    st32 = st64 = P.fresh_state() if c.use_valuenorm else None
    for inp, out, st in steps:
        r32, r64 = P.restate(inp, c, torch.float32, st32), P.restate(inp, c, torch.float64, st64)
        # float32: the reference's own ops in its order. Equal, or within 1 ulp where a reduction's order is torch's choice per shape
        for k in ("action_log_probs", "imp_weights", "grad_logits", "grad_values", "policy_loss", "dist_entropy", "value_loss", "ratio_mean"):
            assert _ulps32(r32[k], out[k]).max() <= 1, (k, _ulps32(r32[k], out[k]).max())
        # float64 against the reference's float32 run: the per-element bound with the reference's own error class
        for k, scale in (("action_log_probs", 1.0), ("imp_weights", 1.0), ("grad_logits", r64["denom_policy"]), ("grad_values", r64["denom_value"])):
            assert P.row_err(out[k] * scale, r64[k] * scale).max() <= P.C_REF, k
        b = P.scalar_bounds(r64, P.C_REF)
        for k in ("policy_loss", "dist_entropy", "value_loss", "ratio_mean"):
            assert abs(float(out[k]) - float(r64[k])) <= b[k] + P.U * abs(float(r64[k])), k       # + the float32 rounding of the reference's scalar itself
        if c.use_valuenorm:
            for k in st:
                np.testing.assert_array_equal(r32["state"][k].reshape(-1), st[k].reshape(-1))
                B = len(inp["returns"])
                tol = (np.log2(B) + 4) * P.U * float(np.abs(inp["returns"] if k != "running_mean_sq" else inp["returns"] ** 2).mean())
                assert abs(float(st[k].reshape(-1)[0]) - float(r64["state"][k].reshape(-1)[0])) <= tol, k
            st32, st64 = r32["state"], r64["state"]


def test_fixture_covers_the_flags_deltas_and_action_counts():
    d = np.load(GOLD)
    flags = np.array([d[n + "_flags"] for n in FIX_CASES])
    assert all(set(flags[:, j]) == {False, True} for j in range(5))
    assert {int(d[n + "_K"]) for n in FIX_CASES} == {5, 25}
    assert {float(d[n + "_cfg"][1]) for n in FIX_CASES if d[n + "_flags"][3]} == {10.0, 0.5}


# ---------------------------------------------------------------------------------------------- the tolerance's source
def test_reference_float32_error_stays_below_the_recorded_constant():
    """C_DEV = 4 * C_REF is what the device gets; C_REF must bound the error of the reference's own float32 arithmetic, re-derived here."""
    worst = 0.0
    for case in P.ALL_CASES:
        inp, c, st = P.case_inputs(case)
        worst = max(worst, P.reference_error(P.restate(inp, c, torch.float32, st), P.restate(inp, c, torch.float64, st)))
    print("float32 restatement vs float64: %.2f units of U * (1 + |x|); C_REF %.0f, C_DEV %.0f" % (worst, P.C_REF, P.C_DEV))
    assert P.C_REF / 2 < worst <= P.C_REF and P.C_DEV == 4 * P.C_REF


# ---------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("case", P.ALL_CASES, ids=lambda c: "%s-%dx%d" % c[:3])
def test_every_decision_is_a_tie_or_has_a_margin(case):
    inp, c, st = P.case_inputs(case)
    gaps = P.decision_gaps(P.restate(inp, c, torch.float64, st)["decisions"], c)
    g32 = P.decision_gaps(P.restate(inp, c, torch.float32, st)["decisions"], c)
    for k, g in gaps.items():
        assert ((g == 0) | (g >= P.MARGIN)).all(), k
        assert ((g == 0) == (g32[k] == 0)).all(), k            # a tie is a tie in float32 and float64 alike
    if case[0] == "ties":
        assert (gaps["d_hi"] == 0).mean() >= 0.2 and (gaps["d_lo"] == 0).mean() >= 0.2 and (gaps["branches"] == 0).mean() >= 0.2
    if case[0] == "edges" and case[2] > 1:
        assert (gaps["surr"] == 0).any()
    if case in P.RATIO_TIE_CASES:                              # rows with the ratio exactly at 1 - clip and at 1 + clip exist
        at = (gaps["ratio_lo"].reshape(-1) == 0) & (gaps["ratio_hi"].reshape(-1) == 0)
        assert at.sum() >= (len(at) // 5 if case[2] > 1 else len(at) * 4 // 5)
        assert (gaps["surr"].reshape(-1)[at] == 0).all()


def test_ratio_tie_cases_are_among_the_cases():
    assert len(P.RATIO_TIE_CASES) == 2 and {c[2] for c in P.RATIO_TIE_CASES} == {1, 25}


# ---------------------------------------------------------------------------------------------- (c)
WRONG = [("symmetric_huber", ("generic", 300, 5, dict(huber_delta=0.5), "ones", "given")),
         ("plain_means", ("generic", 257, 25, dict(), "mixed", "given")),
         ("stale_stats", ("generic", 257, 25, dict(valuenorm=True), "mixed", "given")),
         ("unmasked_logits", ("generic", 257, 25, dict(), "mixed", "given")),
         ("masked_leak", ("edges", 260, 25, dict(), "mixed", "given")),
         ("clamp_leak", ("generic", 257, 25, dict(), "mixed", "given")),
         ("first_max", ("ties", 256, 9, dict(huber=False), "mixed", "given"))]


@pytest.mark.parametrize("variant,case", WRONG, ids=[w[0] for w in WRONG])
def test_inputs_tell_the_truth_from_a_wrong_variant(variant, case):
    assert case in P.ALL_CASES
    inp, c, st = P.case_inputs(case)
    ref, bad = P.restate(inp, c, torch.float64, st), P.restate(inp, c, torch.float64, st, variant=variant)
    b = P.scalar_bounds(ref, P.C_DEV)
    scalar = any(abs(float(bad[k]) - float(ref[k])) > b[k] for k in b)
    rows = 0.0
    for k, scale in (("grad_logits", ref["denom_policy"]), ("grad_values", ref["denom_value"])):
        e = P.row_err(bad[k] * scale, ref[k] * scale).reshape(len(inp["logits"]), -1).max(axis=1)
        rows = max(rows, float((e > P.C_DEV).mean()))
    assert scalar or rows >= 0.10, (variant, scalar, rows)


# ---------------------------------------------------------------------------------------------- (d)
def test_symbols_are_exported_and_the_plan_matches_the_header():
    lib = _lib.load()
    assert {"gmpe_ppo_loss", "gmpe_ppo_loss_workspace_bytes"} <= set(_lib.SYMBOLS) & abi_lib.exported()
    assert abi_lib.layout(_lib.GmpePpoLossPlan) == abi_lib.mirror_layout(_lib.GmpePpoLossPlan)      # every field by its header name, at the header's offset
    assert _lib.PPO_MAX_ACTIONS >= 64 and abi_lib.constant("GMPE_PPO_MAX_ACTIONS") == _lib.PPO_MAX_ACTIONS
    assert abi_lib.constant("GMPE_PPO_NUM_OUT") == _lib.PPO_NUM_OUT == len(_lib.PPO_OUT)
    assert abi_lib.constant("GMPE_ABI_VERSION") == 3
    n = C.c_size_t()
    assert lib.gmpe_ppo_loss_workspace_bytes(1000, C.byref(n)) == 0 and n.value >= 4 * 7 * 8 and n.value % 8 == 0
    assert lib.gmpe_ppo_loss_workspace_bytes(0, C.byref(n)) == -1


def _plan(**over):
    p = _lib.GmpePpoLossPlan()
    p.rows, p.n_actions, p.flags = 10, 5, 15
    p.clip_param, p.huber_delta, p.entropy_coef, p.beta, p.epsilon = 0.2, 10.0, 0.01, 0.99999, 1e-5
    for k in ("logits", "values", "actions", "old_action_log_probs", "adv_targ", "value_preds", "returns", "active_masks", "out", "grad_logits",
              "grad_values", "workspace"):
        setattr(p, k, 0x10000)
    p.workspace_bytes = 1 << 20
    for k, v in over.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("bad", [dict(rows=0), dict(n_actions=0), dict(n_actions=65), dict(flags=32), dict(logits=None), dict(values=None),
                                 dict(actions=None), dict(active_masks=None), dict(out=None), dict(grad_logits=None), dict(grad_values=None),
                                 dict(workspace=None), dict(workspace_bytes=8), dict(workspace=0x10004), dict(flags=16), dict(running_mean=0x10000),
                                 dict(actions_int64=2), dict(actions_int64=1, actions=0x10004), dict(logits=0x10002), dict(out=0x10004),
                                 dict(clip_param=-0.1), dict(huber_delta=float("nan")), dict(flags=16, running_mean=0x10000, running_mean_sq=0x10000)],
                         ids=lambda b: "-".join(b))
def test_c_entry_point_refuses_bad_plans_before_any_device_call(bad):
    lib = _lib.load()
    assert lib.gmpe_ppo_loss(0, C.byref(_plan(**bad)), None) == -1
    assert lib.gmpe_last_error().decode().startswith("gmpe_ppo_loss:")
    assert lib.gmpe_ppo_loss(0, None, None) == -1


def _sample(B=6, K=5, **over):
    z = lambda *s: torch.zeros(*s)
    f = dict(actions=z(B, 1), value_preds=z(B, 1), returns=z(B, 1), active_masks=torch.ones(B, 1), old_action_log_probs=z(B, 1), adv_targ=z(B, 1),
             available_actions=torch.ones(B, K))
    f.update(over)
    return f


def test_python_layer_refuses_what_it_does_not_support():
    args = types.SimpleNamespace(use_valuenorm=False)
    lg, vl = torch.zeros(6, 5), torch.zeros(6, 1)
    assert gmpe.ppo_losses is gmpe.ppo_loss.ppo_losses
    with pytest.raises(NotImplementedError, match="use_popart"):
        gmpe.ppo_losses(lg, vl, _sample(), types.SimpleNamespace(use_popart=True, use_valuenorm=False))
    with pytest.raises(ValueError, match="above the supported"):
        gmpe.ppo_losses(torch.zeros(6, 65), vl, _sample(K=65), args)
    with pytest.raises(NotImplementedError, match="single Discrete head"):
        gmpe.ppo_losses(lg, vl, _sample(actions=torch.zeros(6, 2)), args)
    with pytest.raises(ValueError, match="actions must be"):
        gmpe.ppo_losses(lg, vl, _sample(actions=torch.zeros(6, 1, dtype=torch.int32)), args)
    with pytest.raises(ValueError, match="returns must have shape"):
        gmpe.ppo_losses(lg, vl, _sample(returns=torch.zeros(5, 1)), args)
    with pytest.raises(ValueError, match="adv_targ must be"):
        gmpe.ppo_losses(lg, vl, _sample(adv_targ=torch.zeros(6, 1, dtype=torch.float64)), args)
    with pytest.raises(ValueError, match="available_actions must be"):
        gmpe.ppo_losses(lg, vl, _sample(available_actions=torch.ones(6, 4)), args)
    with pytest.raises(ValueError, match="values must be"):
        gmpe.ppo_losses(lg, torch.zeros(5, 1), _sample(), args)
    with pytest.raises(ValueError, match="logits must be"):
        gmpe.ppo_losses(torch.zeros(6, 5, dtype=torch.int64), vl, _sample(), args)
    with pytest.raises(ValueError, match="16-tuple"):
        gmpe.ppo_losses(lg, vl, (1, 2, 3), args)
    with pytest.raises(ValueError, match="holds no"):
        gmpe.ppo_losses(lg, vl, (None,) * 16, args)
    with pytest.raises(ValueError, match="value_normalizer"):
        gmpe.ppo_losses(lg, vl, _sample(), types.SimpleNamespace(use_valuenorm=True))
    wide = types.SimpleNamespace(running_mean=torch.zeros(2), running_mean_sq=torch.zeros(2), debiasing_term=torch.zeros(()), norm_axes=1,
                                 per_element_update=False)
    per = types.SimpleNamespace(running_mean=torch.zeros(1), running_mean_sq=torch.zeros(1), debiasing_term=torch.zeros(()), norm_axes=1,
                                per_element_update=True)
    for vn in (wide, per, object()):
        with pytest.raises(NotImplementedError):
            gmpe.ppo_losses(lg, vl, _sample(), types.SimpleNamespace(use_valuenorm=True), value_normalizer=vn)
    with pytest.raises(ValueError, match="no CPU fallback"):                # everything else in order: the arrays are not on a device
        gmpe.ppo_losses(lg, vl, _sample(), args)
