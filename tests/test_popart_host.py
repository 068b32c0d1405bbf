"""Host side of the PPO loss with PopArt (include/gmpe.h gmpe_ppo_loss_popart, gmpe.ppo_losses_popart), no GPU:
(a) the restatements of tests/popart_lib.py reproduce the reference's own run (tests/golden/popart_loss.npz, made by tests/golden/make_popart_fixture.py:
    GR_MAPPO.ppo_update with use_popart on a stub policy whose critic ends in a real PopArt(H, 1), three minibatches);
(b) every cheap wrong variant differs from that run by at least ten times the tolerance the device is tested with, in at least one case;
(c) the plan's layout against the C header, the exported symbols, and the refusals of both layers, which need no device;
and the error of the reference's own float32 arithmetic on grad_features, which the existing C_DEV must cover (popart_lib.C_ROW).

On `exact`: the first minibatch's dot products are exact in any order, so its values and everything after them are compared bit for bit. PopArt.update
then leaves weights (W * s) / s', which are no longer short: from the second minibatch on a float32 dot product rounds, its bits depend on the order of
the sum, and values are compared with the dot-product bound while everything after them is evaluated AT the run's own values and compared bit for bit
again. The six PopArt tensors never depend on the values and are bit for bit in all three minibatches."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import abi_lib
import gmpe
import popart_lib as PL
import ppo_loss_lib as P
from gmpe import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "popart_loss.npz")
FIX_CASES = ("g8", "g64", "exact")


def fixture_case(d, name):
    """(cfg, K, H, initial PopArt arrays, [(inputs, outputs, PopArt arrays after)] for the three minibatches) of one fixture case."""
    clip, delta, ent = (float(x) for x in d[name + "_cfg"])
    pm, vm, clipped, huber = (bool(x) for x in d[name + "_flags"])
    c = PL.cfg(clip_param=clip, huber_delta=delta, entropy_coef=ent, pm=pm, vm=vm, clipped=clipped, huber=huber)
    init = {k: d["%s_init_%s" % (name, k)] for k in PL.STATE}
    steps = []
    for i in range(3):
        pre = "%s_%d_" % (name, i)
        inp = {k[len(pre) + 3:]: d[k] for k in d.files if k.startswith(pre + "in_")}
        out = {k[len(pre):]: d[k] for k in d.files if k.startswith(pre) and not k.startswith(pre + "in_") and not k.startswith(pre + "state_")}
        st = {k[len(pre) + 6:]: d[k] for k in d.files if k.startswith(pre + "state_")}
        steps.append((inp, out, st))
    return c, int(d[name + "_K"]), int(d[name + "_H"]), init, steps


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).reshape(-1).view(np.uint32)


def check_against_run(got, out, st_after, ref, inp, cc, what, exact_rows):
    """`got` (a float32 restatement, or the device) against the reference's run `out` / `st_after`; ref: the float64 restatement AT got's values.
    exact_rows: the per-row arrays must be the run's bits (the caller made the values equal first); else they get C * U * (1 + |x|)."""
    B = len(inp["returns"])
    if exact_rows:
        for k in PL.STATE:
            assert np.array_equal(bits(got["state"][k]), bits(st_after[k])), (what, k)
        assert np.array_equal(bits(got["grad_features"]), bits(out["grad_features"])), what
    for k, terms in (("grad_weight", ref["abs_grad_weight"]), ("grad_bias", ref["abs_grad_bias"])):
        tol = PL.sum_bound(B, terms) + U32 * np.abs(ref[k])
        err = np.abs(np.asarray(got[k], np.float64).reshape(ref[k].shape) - np.asarray(out[k], np.float64).reshape(ref[k].shape))
        assert (err <= 2 * tol).all(), (what, k, float((err / tol).max()))           # both sides are float32 sums of the same terms
    b = P.scalar_bounds(ref, cc)
    for k in ("policy_loss", "dist_entropy", "value_loss", "ratio_mean"):
        assert abs(float(got[k]) - float(out[k])) <= b[k] + P.U * abs(float(ref[k])), (what, k)


U32 = P.U


# ---------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("name", FIX_CASES)
def test_restatements_reproduce_the_reference_run(name):
    c, K, H, st32, steps = fixture_case(np.load(GOLD), name)
    st64 = st32
    for i, (inp, out, st_after) in enumerate(steps):
        B = len(inp["returns"])
        free32 = PL.restate(inp, c, st32, torch.float32)
        free64 = PL.restate(inp, c, st64, torch.float64)
        # the head: any float32 order stays within the dot-product bound of the float64 value; exact in the first minibatch of `exact`
        vb = PL.value_bound(free64)
        assert (np.abs(out["values"].astype(np.float64) - free64["values"]) <= vb).all()
        assert (np.abs(free32["values"].astype(np.float64) - free64["values"]) <= vb).all()
        if name == "exact" and i == 0:
            assert np.array_equal(bits(free32["values"]), bits(out["values"])) and np.array_equal(free64["values"], out["values"].astype(np.float64))
        # everything after the head, at the run's own values
        r32 = PL.restate(inp, c, st32, torch.float32, values=out["values"])
        r64 = PL.restate(inp, c, st32, torch.float64, values=out["values"])
        if name == "exact":
            check_against_run(r32, out, st_after, r64, inp, P.C_REF, "%s[%d]" % (name, i), exact_rows=True)
        else:
            check_against_run(r32, out, st_after, r64, inp, P.C_REF, "%s[%d]" % (name, i), exact_rows=False)
            D = r64["denom_value"]
            assert P.row_err(out["grad_features"] * D, r64["grad_features"] * D).max() <= P.C_REF
            assert P.row_err(r32["grad_features"] * D, out["grad_features"] * D).max() <= 2          # the same float32 ops: a last bit where torch's order is free
            for k in ("mean", "mean_sq", "debiasing_term"):                  # float32 summation noise of the batch means
                assert abs(float(r32["state"][k].reshape(-1)[0]) - float(st_after[k].reshape(-1)[0])) <= PL.stat_tol(inp, k), k
                assert abs(float(free64["state"][k].reshape(-1)[0]) - float(st_after[k].reshape(-1)[0])) <= (i + 1) * PL.stat_tol(inp, k), k
            # the rescaled layer is elementwise: fed the run's own statistics, float32 gives the run's bits and float64 lies within the layer bound
            s32, w32, b32 = PL.rescale_layer(st32["weight"], st32["bias"], st32["stddev"], st_after["mean"], st_after["mean_sq"], torch.float32)
            for got, k in ((s32, "stddev"), (w32, "weight"), (b32, "bias")):
                assert np.array_equal(bits(got), bits(st_after[k])), k
            s64, w64, b64 = PL.rescale_layer(st32["weight"], st32["bias"], st32["stddev"], st_after["mean"], st_after["mean_sq"])
            wb, bb = PL.layer_bounds(st32["weight"], st32["bias"], st32["stddev"], st_after["mean"], s64)
            assert (np.abs(st_after["weight"] - w64) <= wb).all() and (np.abs(st_after["bias"] - b64) <= bb).all()
        # the policy side does not know about PopArt
        assert P.row_err(out["action_log_probs"], r64["action_log_probs"]).max() <= P.C_REF
        assert P.row_err(out["grad_logits"] * r64["denom_policy"], r64["grad_logits"] * r64["denom_policy"]).max() <= P.C_REF
        st32, st64 = st_after, free64["state"]


def test_fixture_covers_what_the_issue_names():
    d = np.load(GOLD)
    assert [(int(d[n + "_H"]), int(d[n + "_K"]), d["%s_0_in_returns" % n].shape[0]) for n in FIX_CASES] == [(8, 25, 96), (64, 5, 96), (64, 5, 128)]
    assert d["g8_flags"].all() and not d["g64_flags"].any()
    for i in range(3):
        r, f = d["exact_%d_in_returns" % i], d["exact_%d_in_features" % i]
        assert (r * 8 == np.round(r * 8)).all() and np.abs(r).max() <= 16 and (f * 4 == np.round(f * 4)).all() and np.abs(f).max() <= 2
    w, b = d["exact_init_weight"], d["exact_init_bias"]
    assert (w * 8 == np.round(w * 8)).all() and np.abs(w).max() <= 1 and (b * 8 == np.round(b * 8)).all()
    for n in FIX_CASES:
        for i in range(3):                                           # the sqrt of step 4 stays real
            assert float(d["%s_%d_state_mean_sq" % (n, i)][0]) - float(d["%s_%d_state_mean" % (n, i)][0]) ** 2 > 0
            assert d["%s_%d_state_stddev" % (n, i)][0] > 1e-4       # and above its clamp: the rescale is a real one


def test_reference_float32_error_of_the_head_gradient_stays_below_the_constant():
    """grad_features gets the existing C_DEV (popart_lib.C_ROW): four times the float32 restatement's own error must fit it."""
    worst = 0.0
    for B, K, H, kw, masks in PL.CASES:
        c = PL.cfg(**kw)
        st = PL.fresh_popart(H)
        for step in range(2):                                        # a fresh layer, then a rescaled one
            inp = PL.family(B, K, H, st, c, seed=step, masks=masks)
            r32 = PL.restate(inp, c, st, torch.float32)
            r64 = PL.restate(inp, c, st, torch.float64, values=r32["values"])
            r32 = PL.restate(inp, c, st, torch.float32, values=r32["values"])
            worst = max(worst, PL.head_error(r32, r64))
            st = r32["state"]
    print("float32 restatement vs float64, D * grad_features: %.2f units of U * (1 + |x|); C_ROW %.0f" % (worst, PL.C_ROW))
    assert 0 < 4 * worst <= PL.C_ROW == P.C_DEV


# ---------------------------------------------------------------------------------------------- (b)
def _worst_ratio(bad, out, st_after, ref, inp, st_in):
    """The largest |wrong variant - the reference's run| / (the tolerance the device is tested with) over the outputs the GPU test compares."""
    D = ref["denom_value"]
    r = [float((np.abs(bad["values"] - out["values"].astype(np.float64)) / PL.value_bound(ref)).max()),
         float(P.row_err(bad["grad_features"] * D, out["grad_features"].astype(np.float64) * D).max() / PL.C_ROW)]
    for k in ("mean", "mean_sq"):
        r.append(abs(float(bad["state"][k].reshape(-1)[0]) - float(st_after[k].reshape(-1)[0])) / PL.stat_tol(inp, k))
    wb, bb = PL.layer_bounds(st_in["weight"], st_in["bias"], st_in["stddev"], st_after["mean"], st_after["stddev"])
    r.append(float((np.abs(bad["state"]["weight"] - st_after["weight"]) / wb).max()))
    r.append(float((np.abs(bad["state"]["bias"] - st_after["bias"]) / bb).max()))
    r.append(abs(float(bad["state"]["stddev"].reshape(-1)[0]) - float(st_after["stddev"][0])) / (PL.C_LAYER * P.U * (1 + float(st_after["stddev"][0]))))
    b = P.scalar_bounds(ref, P.C_DEV)["value_loss"] + P.U * abs(float(ref["value_loss"]))
    r.append(abs(float(bad["value_loss"]) - float(out["value_loss"])) / b)
    return max(r)


@pytest.mark.parametrize("variant", PL.VARIANTS)
def test_the_run_tells_the_truth_from_a_wrong_variant(variant):
    d = np.load(GOLD)
    worst, truth = 0.0, 0.0
    for name in FIX_CASES:
        c, K, H, st_in, steps = fixture_case(d, name)
        for inp, out, st_after in steps:
            ref = PL.restate(inp, c, st_in, torch.float64, values=out["values"])
            bad = PL.restate(inp, c, st_in, torch.float64, variant=variant, values=None if variant == "post_update_values" else out["values"])
            if variant != "post_update_values":
                bad["values"] = ref["values"]
            worst = max(worst, _worst_ratio(bad, out, st_after, ref, inp, st_in))
            truth = max(truth, _worst_ratio(ref, out, st_after, ref, inp, st_in))
            st_in = st_after
    print("%s: %.1f tolerances away from the reference's run (the restatement itself: %.2f)" % (variant, worst, truth))
    assert truth <= 1.0 and worst >= 10.0, (variant, worst, truth)


# ---------------------------------------------------------------------------------------------- (c)
def test_symbols_are_exported_and_the_plan_matches_the_header():
    lib = _lib.load()
    assert {"gmpe_ppo_loss_popart", "gmpe_ppo_loss_popart_workspace_bytes"} <= set(_lib.SYMBOLS) & abi_lib.exported()
    assert lib.gmpe_abi_version() == 3 and gmpe.config.ABI_VERSION == 3          # an added entry point: the ABI version stays
    PP = _lib.GmpePopartLossPlan
    assert abi_lib.layout(PP) == abi_lib.mirror_layout(PP) and C.sizeof(PP) == 8 + 4 * 4 + 5 * 8 + 28 * 8
    assert abi_lib.constant("GMPE_POPART_MAX_HIDDEN") == _lib.POPART_MAX_HIDDEN == 1024
    assert abi_lib.layout(_lib.GmpePpoLossPlan)[0] == C.sizeof(_lib.GmpePpoLossPlan)   # the existing plan is untouched
    n = C.c_size_t()
    assert lib.gmpe_ppo_loss_popart_workspace_bytes(1000, 64, C.byref(n)) == 0 and n.value >= 4 * (8 + 64) * 8 and n.value % 8 == 0
    for rows, hidden in ((0, 64), (10, 0), (10, 1025)):
        assert lib.gmpe_ppo_loss_popart_workspace_bytes(rows, hidden, C.byref(n)) == -1


REQUIRED = ("logits", "critic_features", "actions", "old_action_log_probs", "adv_targ", "value_preds", "returns", "active_masks", "weight", "bias", "stddev",
            "mean", "mean_sq", "debiasing_term", "weight_out", "bias_out", "stddev_out", "out", "grad_logits", "grad_features", "grad_weight", "grad_bias",
            "workspace")


def _plan(**over):
    p = _lib.GmpePopartLossPlan()
    p.rows, p.n_actions, p.hidden, p.flags = 10, 5, 8, 15
    p.clip_param, p.huber_delta, p.entropy_coef, p.beta, p.epsilon = 0.2, 10.0, 0.01, 0.99999, 1e-5
    for k in REQUIRED:
        setattr(p, k, 0x10000)
    p.workspace_bytes = 1 << 20
    for k, v in over.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("bad", [dict(rows=0), dict(n_actions=0), dict(n_actions=65), dict(hidden=0), dict(hidden=1025), dict(flags=16), dict(flags=32),
                                 dict(actions_int64=2), dict(actions_int64=1, actions=0x10004), dict(critic_features=0x10002), dict(out=0x10004),
                                 dict(workspace_bytes=8), dict(workspace=0x10004), dict(clip_param=-0.1), dict(huber_delta=float("nan")), dict(beta=1.5),
                                 dict(epsilon=0.0)] + [{k: None} for k in REQUIRED], ids=lambda b: "-".join(b))
def test_c_entry_point_refuses_bad_plans_before_any_device_call(bad):
    lib = _lib.load()
    assert lib.gmpe_ppo_loss_popart(0, C.byref(_plan(**bad)), None) == -1
    assert lib.gmpe_last_error().decode().startswith("gmpe_ppo_loss_popart:")
    assert lib.gmpe_ppo_loss_popart(0, None, None) == -1


def test_the_existing_entry_point_still_rejects_unknown_flags():
    from test_ppo_loss_host import _plan as old_plan
    lib = _lib.load()
    assert lib.gmpe_ppo_loss(0, C.byref(old_plan(flags=32)), None) == -1 and lib.gmpe_last_error().decode() == "gmpe_ppo_loss: unknown flags"


def _popart(H=8, **over):
    z = torch.zeros
    p = types.SimpleNamespace(weight=torch.nn.Parameter(z(1, H)), bias=torch.nn.Parameter(z(1)), stddev=torch.ones(1), mean=z(1), mean_sq=z(1),
                              debiasing_term=z(()), beta=0.99999, epsilon=1e-5, norm_axes=1, output_shape=1)
    for k, v in over.items():
        if v is None:
            delattr(p, k)
        else:
            setattr(p, k, v)
    return p


def test_python_layer_refuses_what_it_does_not_support():
    from test_ppo_loss_host import _sample
    args = types.SimpleNamespace(use_popart=True, use_valuenorm=False)
    lg, ft = torch.zeros(6, 5), torch.zeros(6, 8)
    assert gmpe.ppo_losses_popart is gmpe.ppo_loss.ppo_losses_popart and gmpe.PPOPopArtLosses._fields == gmpe.PPOLosses._fields + ("values",)
    with pytest.raises(NotImplementedError, match="use_popart.*ppo_losses_popart"):
        gmpe.ppo_losses(lg, torch.zeros(6, 1), _sample(), types.SimpleNamespace(use_popart=True, use_valuenorm=False))
    with pytest.raises(ValueError, match="use_popart is not set"):
        gmpe.ppo_losses_popart(lg, ft, _sample(), types.SimpleNamespace(use_valuenorm=False), _popart())
    with pytest.raises(ValueError, match="simultaneously"):
        gmpe.ppo_losses_popart(lg, ft, _sample(), types.SimpleNamespace(use_popart=True, use_valuenorm=True), _popart())
    with pytest.raises(ValueError, match="install must be"):
        gmpe.ppo_losses_popart(lg, ft, _sample(), args, _popart(), install="copy")
    with pytest.raises(ValueError, match="above the supported 1024"):
        gmpe.ppo_losses_popart(lg, torch.zeros(6, 1025), _sample(), args, _popart(1025))
    with pytest.raises(ValueError, match="critic_features must be"):
        gmpe.ppo_losses_popart(lg, torch.zeros(5, 8), _sample(), args, _popart())
    with pytest.raises(ValueError, match="popart .* is required"):
        gmpe.ppo_losses_popart(lg, ft, _sample(), args, None)
    for name in PL.STATE:
        with pytest.raises(NotImplementedError, match=r"popart\.%s is missing" % name):
            gmpe.ppo_losses_popart(lg, ft, _sample(), args, _popart(**{name: None}))
        with pytest.raises(ValueError, match=r"popart\.%s must" % name):                                    # dtype: named before the device is touched
            gmpe.ppo_losses_popart(lg, ft, _sample(), args, _popart(**{name: getattr(_popart(), name).detach().double()}))
    with pytest.raises(ValueError, match=r"popart\.weight must have shape \(1, 8\)"):
        gmpe.ppo_losses_popart(lg, ft, _sample(), args, _popart(7))
    with pytest.raises(NotImplementedError, match="only PopArt\\(hidden, 1\\)"):
        gmpe.ppo_losses_popart(lg, ft, _sample(), args, _popart(weight=torch.zeros(2, 8)))
    with pytest.raises(NotImplementedError, match="norm_axes"):
        gmpe.ppo_losses_popart(lg, ft, _sample(), args, _popart(norm_axes=2))
    with pytest.raises(NotImplementedError, match="output_shape"):
        gmpe.ppo_losses_popart(lg, ft, _sample(), args, _popart(output_shape=2))
    with pytest.raises(ValueError, match=r"popart\.mean must have shape"):
        gmpe.ppo_losses_popart(lg, ft, _sample(), args, _popart(mean=torch.zeros(2)))
    with pytest.raises(ValueError, match="returns must have shape"):
        gmpe.ppo_losses_popart(lg, ft, _sample(returns=torch.zeros(5, 1)), args, _popart())
    with pytest.raises(ValueError, match="no CPU fallback"):                # everything else in order: the arrays are not on a device
        gmpe.ppo_losses_popart(lg, ft, _sample(), args, _popart())
