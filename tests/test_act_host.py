"""Host side of the rollout half of the action head (include/gmpe.h gmpe_act_sample, gmpe.sample_actions), no GPU:
(a) the float32 restatement of tests/act_lib.py reproduces the reference's own run (tests/golden/act_head.npz, made by tests/golden/make_act_fixture.py:
    ACTLayer.forward with deterministic=True and sampled) — the mode actions exactly, the log-probs to the measured distance;
(b) the symbol, the plan layout and the ABI version; the refusals of the C entry point and of the Python layer, which need no device;
(c) the sampling rule is a sampler: Pearson's chi-squared of 65 536 draws against the float64 probabilities;
(d) float32 and float64 disagree only on rows whose draw lies at a CDF boundary, and those are few — what ties the device to the float64 yardstick;
(e) the action stream's draws are not the env stream's."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import abi_lib
import gmpe
import act_lib as AL
import oracle_lib as ol
from gmpe import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "act_head.npz")
FIX_CASES = ("a", "b", "c", "d", "e", "f")


def fixture_case(d, name):
    return d[name + "_logits"], (d[name + "_avail"] if bool(d[name + "_has_avail"]) else None)


# ---------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("name", FIX_CASES)
def test_restatement_reproduces_the_reference_run(name):
    """Mode actions: exact. Log-probs: torch forms logsumexp in its own way, and its result differs from log(sum exp(x - max)) + max, rounded once per
    operation, by up to one ulp OF THE LOGSUMEXP; l = x - lse then rounds once more. Measured over the fixture: 2 units of
    ulp(max(|lse|, |l|)) (and up to 2048 ulps of a log-prob near zero, which is why the unit is not the log-prob's own ulp). Asserted: 2."""
    d = np.load(GOLD)
    logits, avail = fixture_case(d, name)
    r32, r64 = AL.restate(logits, avail, None, np.float32), AL.restate(logits, avail, None, np.float64)
    R = np.arange(len(logits))
    np.testing.assert_array_equal(r32["mode"], d[name + "_mode"][:, 0])
    np.testing.assert_array_equal(r64["mode"], d[name + "_mode"][:, 0])
    worst = 0.0
    for key in ("mode", "sampled"):
        a = d[name + "_" + key][:, 0]
        if avail is not None:
            assert (avail[R, a] != 0).all()                                   # the reference's sampler never leaves the availability either
        dist = AL.lse_units(r32["l"][R, a], d[name + "_%s_log_probs" % key][:, 0], logits[R, a], r64["l"][R, a])
        worst = max(worst, float(dist.max()))
    print("float32 restatement vs the reference's log-probs: %.1f units of ulp(max(|lse|, |l|))" % worst)
    assert worst <= 2.0


def test_fixture_covers_the_action_counts_availability_and_stop_rows():
    d = np.load(GOLD)
    assert {int(d[n + "_K"]) for n in FIX_CASES} == {5, 25}
    assert {(int(d[n + "_K"]), bool(d[n + "_has_avail"])) for n in FIX_CASES} == {(5, True), (5, False), (25, True), (25, False)}
    for n in FIX_CASES:
        if bool(d[n + "_has_avail"]):
            av, K = d[n + "_avail"], int(d[n + "_K"])
            stop = (av.sum(1) == 1) & (av[:, K // 2] == 1)
            assert stop.sum() >= 10
            assert (d[n + "_mode"][stop, 0] == K // 2).all() and (d[n + "_sampled"][stop, 0] == K // 2).all()
            assert (d[n + "_mode_log_probs"][stop, 0] == 0).all() and (d[n + "_sampled_log_probs"][stop, 0] == 0).all()
        assert (d[n + "_mode"] != d[n + "_sampled"]).any()


# ---------------------------------------------------------------------------------------------- (b)
def test_symbol_is_exported_and_the_plan_matches_the_header():
    lib = _lib.load()
    assert "gmpe_act_sample" in _lib.SYMBOLS and "gmpe_act_sample" in abi_lib.exported()
    assert abi_lib.layout(_lib.GmpeActPlan) == abi_lib.mirror_layout(_lib.GmpeActPlan)      # every field by its header name, at the header's offset
    assert C.sizeof(_lib.GmpeActPlan) == 8 + 6 * 4 + 3 * 8 + 8 * 8
    assert abi_lib.constant("GMPE_ABI_VERSION") == 3 and lib.gmpe_abi_version() == 3
    assert ("int", "gmpe_act_sample", ["int", "const gmpe_act_plan*", "void*"]) in abi_lib.prototypes()
    assert gmpe.sample_actions is gmpe.act.sample_actions


def test_new_kernels_use_no_scratch():
    scratch = abi_lib.scratch("act", "k_act")
    assert len(scratch) == 3 and set(scratch.values()) == {0}                     # the 16-byte and the 4-byte row kernel, the counter's one thread


def _plan(**over):
    p = _lib.GmpeActPlan()
    p.rows, p.n_actions, p.num_agents, p.stop_action = 10, 5, 3, 2
    for k in ("logits", "action_idx", "log_probs"):
        setattr(p, k, 0x10000)
    for k, v in over.items():
        setattr(p, k, v)
    return p


BAD = [(dict(rows=0), "rows"), (dict(n_actions=0), "n_actions"), (dict(n_actions=65), "n_actions"), (dict(num_agents=0), "num_agents"),
       (dict(stop_action=-1), "stop_action"), (dict(stop_action=5), "stop_action"), (dict(deterministic=2), "deterministic"),
       (dict(reserved=1), "reserved"), (dict(available_actions=0x10000, dones_prev=0x10000), "dones_prev"), (dict(logits=None), "logits"),
       (dict(action_idx=None), "action_idx"), (dict(log_probs=None), "log_probs"), (dict(logits=0x10002), "aligned"),
       (dict(actions_i64=0x10004), "aligned"), (dict(draw_dev=0x10004), "aligned"), (dict(actions_f32=0x10001), "aligned")]


@pytest.mark.parametrize("bad,word", BAD, ids=["-".join(b[0]) + "-" + str(i) for i, b in enumerate(BAD)])
def test_c_entry_point_refuses_bad_plans_before_any_device_call(bad, word):
    lib = _lib.load()
    assert lib.gmpe_act_sample(0, C.byref(_plan(**bad)), None) == -1
    msg = lib.gmpe_last_error().decode()
    assert msg.startswith("gmpe_act_sample:") and word in msg, msg
    assert lib.gmpe_act_sample(0, None, None) == -1


def test_python_layer_refuses_what_it_does_not_support():
    kw = dict(seed=1, num_agents=3, draw=0)
    lg = torch.zeros(6, 5)
    with pytest.raises(NotImplementedError, match="single Discrete head"):
        gmpe.sample_actions([lg, lg], **kw)
    with pytest.raises(NotImplementedError, match="single Discrete head"):
        gmpe.sample_actions(torch.zeros(6, 2, 5), **kw)
    with pytest.raises(ValueError, match="logits must be"):
        gmpe.sample_actions(torch.zeros(6, 5, dtype=torch.int64), **kw)
    with pytest.raises(ValueError, match="n_actions = 65 is above the supported"):
        gmpe.sample_actions(torch.zeros(6, 65), **kw)
    with pytest.raises(ValueError, match="logits must be contiguous"):
        gmpe.sample_actions(torch.zeros(5, 6).t(), **kw)
    with pytest.raises(ValueError, match="available_actions and dones_prev"):
        gmpe.sample_actions(lg, torch.ones(6, 5), dones_prev=torch.zeros(6, dtype=torch.uint8), **kw)
    with pytest.raises(ValueError, match="available_actions must be a float32 tensor of shape"):
        gmpe.sample_actions(lg, torch.ones(6, 4), **kw)
    with pytest.raises(ValueError, match="available_actions must be contiguous"):
        gmpe.sample_actions(lg, torch.ones(5, 6).t(), **kw)
    with pytest.raises(ValueError, match="dones_prev must be"):
        gmpe.sample_actions(lg, dones_prev=torch.zeros(5, dtype=torch.uint8), **kw)
    with pytest.raises(ValueError, match="stop_action"):
        gmpe.sample_actions(lg, dones_prev=torch.zeros(6, dtype=torch.uint8), stop_action=5, **kw)
    with pytest.raises(ValueError, match="stop_action is read with dones_prev"):
        gmpe.sample_actions(lg, stop_action=2, **kw)
    with pytest.raises(ValueError, match="num_agents"):
        gmpe.sample_actions(lg, seed=1, num_agents=0, draw=0)
    with pytest.raises(ValueError, match="draw_dev must be"):
        gmpe.sample_actions(lg, draw_dev=torch.zeros(1, dtype=torch.int32), **kw)
    with pytest.raises(ValueError, match="unknown out entries"):
        gmpe.sample_actions(lg, out=dict(values=torch.zeros(6)), **kw)
    with pytest.raises(ValueError, match=r"out\['action_idx'\] must be"):
        gmpe.sample_actions(lg, out=dict(action_idx=torch.zeros(6, dtype=torch.int64)), **kw)
    with pytest.raises(ValueError, match="no CPU fallback"):                # everything else in order: the arrays are not on a device
        gmpe.sample_actions(lg, **kw)


# ---------------------------------------------------------------------------------------------- (c)
CHI2_SEED = 20260117
CHI2_Q999_DF17 = 40.790           # the 0.999 quantile of chi-squared with 17 degrees of freedom


def test_inverse_cdf_rule_samples_the_distribution():
    """65 536 rows share one logit row of K = 25 with 7 entries masked; the draws are the action stream's own (3 agents, one draw counter). Proved on the
    float32 restatement, to which tests/test_gpu_act.py ties the device row by row."""
    B, K, A = 65536, 25, 3
    rng = np.random.RandomState(5)
    row = (rng.randn(K) * 1.5).astype(np.float32)
    av = np.ones(K, np.float32)
    av[[0, 3, 4, 11, 12, 19, 24]] = 0.0
    logits, avail = np.tile(row, (B, 1)), np.tile(av, (B, 1))
    u = AL.draws(CHI2_SEED, 0, A, 0, B)
    r32, r64 = AL.restate(logits, avail, u, np.float32), AL.restate(logits[:1], avail[:1], None, np.float64)
    counts = np.bincount(r32["actions"], minlength=K)
    assert (counts[av == 0] == 0).all() and counts.sum() == B
    p = r64["p"][0][av != 0]
    assert abs(p.sum() - 1.0) < 1e-12 and B * p.min() > 5                       # every expected count is large enough for the statistic
    chi2 = float((((counts[av != 0] - B * p) ** 2) / (B * p)).sum())
    print("chi-squared %.2f with %d degrees of freedom (0.999 quantile %.2f)" % (chi2, len(p) - 1, CHI2_Q999_DF17))
    assert len(p) - 1 == 17 and chi2 < CHI2_Q999_DF17


# ---------------------------------------------------------------------------------------------- (d)
@pytest.mark.parametrize("case", AL.CASES, ids=lambda c: "%s-%dx%d-A%d-%s" % (c[0], c[1], c[2], c[3], c[5]))
def test_float32_and_float64_agree_off_the_cdf_boundaries(case):
    fam, B, K, A, base, kind = case
    logits, avail = AL.family(fam, B, K, seed=0, avail=kind)
    u = AL.draws(AL.SEED, base, A, AL.DRAW, B)
    r32, r64 = AL.restate(logits, avail, u, np.float32), AL.restate(logits, avail, u, np.float64)
    assert float(np.abs(r32["cdf"].astype(np.float64) - r64["cdf"]).max()) <= (K + 4) * 2.0 ** -23
    amb, allowed = AL.ambiguity(r64, u, K)
    print("ambiguous rows: %d of %d" % (amb.sum(), B))
    assert amb.sum() <= AL.AMBIGUOUS_MAX * B
    assert (r32["actions"][~amb] == r64["actions"][~amb]).all()
    assert allowed[np.arange(B), r32["actions"]].all()
    if avail is not None:
        some = avail.any(axis=1)
        assert (avail[np.arange(B), r32["actions"]][some] != 0).all()              # never an unavailable action
    assert (r32["actions"] != r32["mode"]).any() or K == 1 or B == 1


def test_ambiguous_rows_stay_few_over_many_draws():
    """The bound above over 65 536 rows of the widest head, where a row has the most boundaries."""
    B, K, A = 65536, 64, 10
    logits, _ = AL.family("unit", 1024, K, seed=3, avail="none")
    logits = np.tile(logits, (B // 1024, 1))
    u = AL.draws(AL.SEED, 77, A, 5, B)
    r32, r64 = AL.restate(logits, None, u, np.float32), AL.restate(logits, None, u, np.float64)
    amb, allowed = AL.ambiguity(r64, u, K)
    print("ambiguous rows: %d of %d (%.3f %%)" % (amb.sum(), B, 100.0 * amb.mean()))
    assert amb.mean() <= AL.AMBIGUOUS_MAX
    assert (r32["actions"][~amb] == r64["actions"][~amb]).all() and allowed[np.arange(B), r32["actions"]].all()


# ---------------------------------------------------------------------------------------------- (e)
def test_action_stream_is_not_the_env_stream():
    lib = ol.load()
    seen = set()
    for seed, env in ((1, 0), (AL.SEED, 12345)):
        for k in list(range(256)) + [2 ** 31, 2 ** 32 + 5, 2 ** 62]:
            a, b = lib.gmpo_philox_uniform(seed, env, k), lib.gmpo_philox_uniform(seed, env, AL.TOP | k)
            assert a != b and 0.0 <= b < 1.0
            seen.update((a, b))
    assert len(seen) == 2 * 2 * 259                                             # all distinct: no draw of one stream is a draw of the other
    # the draws act_lib hands out are these: agent a of env e at call d reads counter 2^63 | (d * A + a)
    u = AL.draws(7, 100, 3, 4, 7, row0=2)
    want = [lib.gmpo_philox_uniform(7, 100 + r // 3, AL.TOP | (4 * 3 + r % 3)) for r in range(2, 9)]
    assert list(u) == want
