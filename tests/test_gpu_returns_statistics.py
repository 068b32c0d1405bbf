"""The mean and population std behind the normalised advantages (csrc/gmpe_returns.hip: Welford per lane, Chan merges in the wave butterfly,
k_adv_stats' strided merge) held bit for bit instead of within 1e-5, on inputs that tell a wrong accumulation apart.

k_adv_normalize is fdiv_rn(fsub_rn(a, mean32), den32) and NumPy's float32 (adv - m) / d is the same two correctly rounded operations, so with the
device's own raw advantages (asserted bit for bit first) the whole normalised array is a function of (mean32, den32). returns_lib.candidate_pairs
lists the pairs a correct double accumulation can end at (+-1 ulp around the exact mean, +-2 ulps around float32(std) + 1e-5f; the derivation is in
its docstring) and returns_lib.match_pair finds the one that reproduces the device array. tests/test_returns_host.py shows on the CPU that ten
wrong variants of the kernel's order (float32 accumulators, the wrong Chan weight, ddof 1, dropped partials ...) leave that set on these inputs.

Both Welford call sites are driven with prescribed raw advantages (returns_lib.prescribed_inputs): k_advantages through the advantages-only path,
k_returns through the Monte-Carlo recurrence with masks = 0. Further: rollout lengths at and around the unroll factor for every branch of the
recurrence, and the plan's stride > lanes through the C entry point."""
import ctypes as C

import numpy as np
import pytest

import gmpe
from gmpe import _lib
import returns_lib as R

pytestmark = pytest.mark.gpu
PATHS = ("advantages", "recurrence")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _device_run(case, path, in_place):
    """-> (raw advantages, normalised advantages) [T, lanes] of a case through one call site; in place: one array for both, so no raw advantages."""
    import torch
    a, am = R.stat_cases()[case]
    T, L = a.shape
    g = lambda x: torch.as_tensor(np.array(x), device="cuda")                       # a copy: the cases are read-only arrays
    p = {k: g(v) for k, v in R.prescribed_inputs(a, path).items()}
    adv = torch.full((T, L, 1), -7.0, device="cuda")
    nrm = adv if in_place else torch.full((T, L, 1), -7.0, device="cuda")
    kw = dict(advantages=adv, normalized=nrm, active_masks=g(am.reshape(T + 1, L, 1)))
    if path == "advantages":
        gmpe.engine.compute_returns(None, None, p["value_preds"], p["returns"], advantages_only=True, **kw)
    else:
        gmpe.engine.compute_returns(p["rewards"], p["masks"], p["value_preds"], p["returns"], p["next_value"], gamma=0.99, gae_lambda=0.95,
                                    use_gae=False, use_proper_time_limits=False, **kw)
    torch.cuda.synchronize()
    return (None if in_place else adv.cpu().numpy().reshape(T, L)), nrm.cpu().numpy().reshape(T, L)


@pytest.fixture(scope="module")
def outputs():
    """case -> every path of it, run once and shared among the tests of this module: {(path, in_place): (adv, normalized)}."""
    done = {}

    def get(case):
        if case not in done:
            done[case] = {(p, i): _device_run(case, p, i) for p in PATHS for i in (False, True)}
        return done[case]
    return get


def _common(case, outputs):
    """What every case asserts but the statistic itself: the raw advantage bits, both call sites the same bits, in place the same bits."""
    a, am = R.stat_cases()[case]
    out = outputs(case)
    for p in PATHS:
        assert R._same_bits(out[p, False][0], a), "%s %s: the raw advantages are not the prescribed ones" % (case, p)
        assert R._same_bits(out[p, True][1], out[p, False][1]), "%s %s: in place differs" % (case, p)
    assert R._same_bits(out["advantages", False][1], out["recurrence", False][1]), "%s: the two call sites differ" % case
    return a, am, out


@pytest.mark.parametrize("case", [k for k in R.stat_cases() if k not in R.EXACT_CASES])
def test_normalised_advantages_are_one_candidate_pair_bit_for_bit(case, outputs):
    """One candidate reproduces the device array, and it is the pair the float64 emulation of the kernel's order ends at on the host."""
    a, am, out = _common(case, outputs)
    pairs = R.candidate_pairs(*R.stats64(a, am))
    for p in PATHS:
        adv, nrm = out[p, False]
        off = R.match_pair(_bits(adv), _bits(nrm), pairs)
        print("%s %s: (dm, dd) = %r" % (case, p, off))
        assert off is not None, "%s %s: no (mean32, den32) within +-1 / +-2 ulps of the exact statistics reproduces the normalised advantages" % (case, p)
        assert off == R.KERNEL_ORDER_OFFSETS, "%s %s: inside the candidates, but not where the kernel's own order lands on the host" % (case, p)
    if case == "nan":
        nrm = out["advantages", False][1]
        assert (np.isnan(nrm) == np.isnan(a)).all()                                  # NaN exactly at the NaN advantages ...
        idle = (am[:-1] == 0) & np.isfinite(a)
        assert idle.any() and np.isfinite(nrm[idle]).all()                           # ... and a number at the inactive finite ones (1e30 among them)
        assert (np.isinf(nrm) == np.isinf(a)).all()


@pytest.mark.parametrize("case", R.EXACT_CASES)
def test_constant_active_advantages_normalise_exactly(case, outputs):
    """One distinct active value: mean = that float32, std = 0, den = float32(1e-5) exactly. The inactive entries differ, so they show both."""
    a, am, out = _common(case, outputs)
    idle = am[:-1] == 0
    assert idle.any() and (a[idle] != R.CONST_VALUE).all()
    for p in PATHS:
        nrm = out[p, False][1]
        assert (_bits(nrm[~idle]) == 0).all(), "%s %s" % (case, p)                   # +0.0
        np.testing.assert_array_equal(_bits(nrm), _bits(R.normalize32(a, R.CONST_VALUE, np.float32(1e-5))), err_msg="%s %s" % (case, p))


DENORM = R.DENORM


@pytest.mark.parametrize("T", R.STEP_TS)
def test_rollout_lengths_around_the_unroll_factor_in_every_branch(T):
    """T = 8, 16 (no tail) and 9, 17 (a tail of one step) x GAE x proper time limits x denormaliser with random masks: returns, value_preds and raw
    advantages against the NumPy restatement bit for bit, and k_advantages on the result gives the same advantage bits. The normalised advantages of
    either call site, after every template of the recurrence, are one candidate pair bit for bit as well (tests/test_returns_host.py shows that
    these advantages stay inside the candidates' limits)."""
    import torch
    lanes = R.BRANCH_LANES
    d = R.branch_inputs(T, lanes)
    g = lambda k: torch.as_tensor(d[k], device="cuda").contiguous()
    for gae in (True, False):
        for proper in (False, True):
            for n in (False, True):
                den = DENORM if n else None
                norm = tuple(torch.tensor([x], device="cuda") for x in DENORM) if n else None
                vp, ret = g("value_preds"), g("returns")
                adv, nrm = (torch.full((T, lanes, 1), -7.0, device="cuda") for _ in range(2))
                gmpe.engine.compute_returns(g("rewards"), g("masks"), vp, ret, g("next_value"), gamma=0.99, gae_lambda=0.95, use_gae=gae,
                                            use_proper_time_limits=proper, bad_masks=g("bad_masks"), denorm=norm, advantages=adv,
                                            active_masks=g("active_masks"), normalized=nrm)
                adv2, nrm2 = (torch.full((T, lanes, 1), -7.0, device="cuda") for _ in range(2))
                gmpe.engine.compute_returns(None, None, vp, ret, advantages_only=True, denorm=norm, advantages=adv2, active_masks=g("active_masks"),
                                            normalized=nrm2)
                torch.cuda.synchronize()
                eret, evp, eadv = R.branch_expectations(d, gae, proper, den)
                label = "T=%d gae=%d proper=%d norm=%d" % (T, gae, proper, n)
                np.testing.assert_array_equal(_bits(ret.cpu().numpy()), _bits(eret), err_msg=label)
                np.testing.assert_array_equal(_bits(vp.cpu().numpy()), _bits(evp), err_msg=label)
                np.testing.assert_array_equal(_bits(adv.cpu().numpy()), _bits(eadv), err_msg=label)
                np.testing.assert_array_equal(_bits(adv2.cpu().numpy()), _bits(eadv), err_msg=label)
                pairs = R.candidate_pairs(*R.stats64(eadv, d["active_masks"]))
                for site, x in (("k_returns", nrm), ("k_advantages", nrm2)):
                    x = x.cpu().numpy()
                    assert np.isfinite(x).all(), label                                # every entry written, by a finite statistic
                    off = R.match_pair(_bits(eadv), _bits(x), pairs)
                    print("%s %s: (dm, dd) = %r" % (label, site, off))
                    assert off is not None, "%s %s: no candidate pair reproduces the normalised advantages" % (label, site)
                    assert off == R.KERNEL_ORDER_OFFSETS, "%s %s" % (label, site)


# ------------------------------------------------------------------------------------------------ stride > lanes, through the C entry point
SENTINEL = np.float32(-777.25)
_SLABS = (("rewards", 0), ("masks", 1), ("bad_masks", 1), ("value_preds", 1), ("returns", 1), ("active_masks", 1), ("advantages", 0), ("normalized", 0))


def _plan_run(torch, d, T, lanes, stride, flags, denorm):
    """gmpe_compute_returns on [rows, stride] slabs pre-filled with SENTINEL, the inputs in the lane columns -> {name: [rows, stride] array}."""
    dev = "cuda"
    t = {}
    for k, extra in _SLABS:
        t[k] = torch.full((T + extra, stride), float(SENTINEL), device=dev)
        if k in d:
            t[k][:, :lanes] = torch.as_tensor(d[k].reshape(T + extra, lanes), device=dev)
    t["next_value"] = torch.full((1, stride), float(SENTINEL), device=dev)
    t["next_value"][0, :lanes] = torch.as_tensor(d["next_value"].reshape(lanes), device=dev)
    ws = torch.empty(gmpe.engine.returns_workspace_bytes(lanes), dtype=torch.uint8, device=dev)
    mean, std = (torch.tensor([x], device=dev) for x in DENORM)
    p = _lib.GmpeReturnsPlan()
    p.num_steps, p.flags, p.lanes, p.stride, p.gamma, p.gae_lambda = T, flags, lanes, stride, 0.99, 0.95
    for k in ("rewards", "masks", "bad_masks", "value_preds", "returns", "next_value", "advantages", "active_masks", "normalized"):
        setattr(p, k, t[k].data_ptr())
    if denorm:
        p.denorm_mean, p.denorm_std = mean.data_ptr(), std.data_ptr()
    p.workspace, p.workspace_bytes = ws.data_ptr(), ws.numel()
    _lib.check(_lib.load().gmpe_compute_returns(0, C.byref(p), C.c_void_p(torch.cuda.current_stream(0).cuda_stream)), "gmpe_compute_returns")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in t.items()}


@pytest.mark.parametrize("lanes", [1, 65])
def test_plan_stride_wider_than_lanes(lanes):
    """stride = lanes + 3: the lane columns are the stride = lanes result bit for bit, the three gap columns keep the sentinel in every array (row T,
    where next_value lands, included)."""
    import torch
    T, gap = 9, 3
    d = R.branch_inputs(T, lanes, seed=400 + lanes)
    runs = (("gae proper denorm", _lib.RETURNS_GAE | _lib.RETURNS_PROPER_TIME_LIMITS, True), ("mc plain", 0, False),
            ("advantages only denorm", _lib.RETURNS_ADVANTAGES_ONLY, True))
    for label, flags, dn in runs:
        tight = _plan_run(torch, d, T, lanes, lanes, flags, dn)
        wide = _plan_run(torch, d, T, lanes, lanes + gap, flags, dn)
        den = DENORM if dn else None
        if flags & _lib.RETURNS_ADVANTAGES_ONLY:
            eret, evp = d["returns"], d["value_preds"]
        else:
            eret, evp = R.np_returns(d["rewards"], d["masks"], d["value_preds"], d["returns"], d["next_value"], 0.99, 0.95,
                                     bool(flags & _lib.RETURNS_GAE), bool(flags & _lib.RETURNS_PROPER_TIME_LIMITS), d["bad_masks"], den)
        exp = dict(returns=eret, value_preds=evp, advantages=R.np_advantages(eret, evp, den))
        for k in ("returns", "value_preds", "advantages"):                           # the tight run is the restatement's, so both are
            np.testing.assert_array_equal(_bits(tight[k]), _bits(exp[k].reshape(tight[k].shape)), err_msg="%s %s" % (label, k))
        assert np.isfinite(tight["normalized"]).all()
        for k, v in wide.items():
            np.testing.assert_array_equal(_bits(v[:, :lanes]), _bits(tight[k]), err_msg="%s %s: lane columns" % (label, k))
            assert (v[:, lanes:] == SENTINEL).all() and v[:, lanes:].shape[1] == gap, "%s %s: a gap column was written" % (label, k)
