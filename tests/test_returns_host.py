"""CPU side of the learner-side rollout kernels (include/gmpe.h gmpe_compute_returns, gmpe_available_actions_from_dones): exported symbols, plan
struct layouts, argument checks of the Python wrappers before any launch, the opt-in policy storage of DeviceRolloutBuffer, and the NumPy
restatement the GPU tests compare with (tests/returns_lib.py) against the reference's own vectors."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import abi_lib
import gmpe
from gmpe import _lib
import returns_lib as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NEW = ("gmpe_returns_workspace_bytes", "gmpe_compute_returns", "gmpe_available_actions_from_dones")


def test_new_symbols_are_exported_and_bound():
    assert set(NEW) <= set(_lib.SYMBOLS) & abi_lib.exported()                  # bound: tests/test_abi_host.py, for every symbol


def test_plan_struct_layouts_match_c_header():
    for P in (_lib.GmpeReturnsPlan, _lib.GmpeAvailPlan):
        assert abi_lib.layout(P) == abi_lib.mirror_layout(P)
    assert [abi_lib.constant("GMPE_RETURNS_" + k) for k in ("GAE", "PROPER_TIME_LIMITS", "ADVANTAGES_ONLY")] == [
        _lib.RETURNS_GAE, _lib.RETURNS_PROPER_TIME_LIMITS, _lib.RETURNS_ADVANTAGES_ONLY] == [1, 2, 4]


def test_workspace_query_and_c_side_validation():
    lib = _lib.load()
    n = C.c_size_t()
    assert lib.gmpe_returns_workspace_bytes(40960, C.byref(n)) == 0 and n.value >= 40960 // 64 * 24
    assert lib.gmpe_returns_workspace_bytes(0, C.byref(n)) == -1
    assert lib.gmpe_compute_returns(0, None, None) == -1
    p = _lib.GmpeReturnsPlan()
    p.num_steps, p.lanes, p.stride = 4, 8, 4                          # stride < lanes
    assert lib.gmpe_compute_returns(0, C.byref(p), None) == -1
    assert b"stride" in lib.gmpe_last_error()
    q = _lib.GmpeAvailPlan(None, None, 8, 25, 4, 0, 4, 8, 200)
    assert lib.gmpe_available_actions_from_dones(0, C.byref(q), None) == -1
    assert gmpe.engine.returns_workspace_bytes(63) == 24 + 8            # one wave partial (count, mean, M2 in double) + mean / std


def _arrays(T=5, N=3, A=2, device="cpu"):
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=device)
    return dict(rewards=z(T, N, A, 1), masks=z(T + 1, N, A, 1), value_preds=z(T + 1, N, A, 1), returns=z(T + 1, N, A, 1), next_value=z(N, A, 1))


@pytest.mark.parametrize("bad, match", [
    (dict(rewards=torch.zeros(6, 3, 2, 1)), "rewards.*shape"),                      # T+1 slots where T are due
    (dict(masks=torch.zeros(6, 3, 2, 1, dtype=torch.float64)), "masks.*float32"),
    (dict(next_value=torch.zeros(3, 3, 1)), "next_value"),
    (dict(returns=torch.zeros(6, 3, 2, 1)[:, :, :1]), "returns.*shape"),
    (dict(advantages=torch.zeros(6, 3, 2, 1)), "advantages.*shape"),
    (dict(denorm=(torch.zeros(2), torch.ones(1))), "denorm mean"),
    (dict(normalized=torch.zeros(5, 3, 2, 1)), "active_masks"),
    (dict(use_proper_time_limits=True), "bad_masks"),
    ({}, "CUDA"),                                                                   # well-formed host tensors: refused for the device
])
def test_compute_returns_refuses_bad_arguments_before_launch(bad, match):
    a = _arrays()
    a.update(bad)
    with pytest.raises(ValueError, match=match):
        gmpe.engine.compute_returns(**a)


@pytest.mark.parametrize("bad, match", [
    (dict(dones=torch.zeros(4, 3, 2, dtype=torch.int32)), "dones"),
    (dict(out=torch.zeros(4, 3, 2, 25, dtype=torch.float64)), "out.*float32"),
    (dict(out=torch.zeros(5, 3, 2, 25)), "out.*shape"),
    (dict(first=4), "first"),
    ({}, "CUDA"),
])
def test_available_actions_refuses_bad_arguments_before_launch(bad, match):
    a = dict(dones=torch.zeros(4, 3, 2, dtype=torch.uint8), out=torch.zeros(4, 3, 2, 25))
    a.update(bad)
    with pytest.raises(ValueError, match=match):
        gmpe.engine.available_actions_from_dones(**a)


class _HostEngine(object):
    """What DeviceRolloutBuffer.__init__ reads from an engine, on the host (no GPU): enough to see which arrays it allocates."""

    def __init__(self, cfg, adj_compact=True):
        self.cfg, self.device, self.adj_compact = cfg, torch.device("cpu"), adj_compact
        self.node_form, self.adj_form = "rows", "compact" if adj_compact else "full"
        self.N, self.A = cfg.num_envs, cfg.num_agents
        self.out = types.SimpleNamespace(info=None)

    def tuning(self):
        return dict(roll=1, split=0)


def test_buffer_without_policy_fields_keeps_todays_storage_spec():
    from gmpe.rollout import DeviceRolloutBuffer, storage_spec
    cfg = gmpe.make_config(num_envs=4, num_agents=3, episode_length=5)
    N, A, E, D, T = 4, 3, cfg.num_entities, cfg.obs_dim, 6
    spec = storage_spec(cfg, T, True, "rows")
    f32 = torch.float32
    assert spec == {"obs": (f32, (T + 1, N, A, D)), "node_obs": (f32, (T + 1, N, A, E, cfg.node_feats)), "_adj": (f32, (T + 1, N, E, E)),
                    "agent_id": (torch.int32, (T + 1, N, A, 1)), "rewards": (f32, (T, N, A, 1)), "dones": (torch.uint8, (T, N, A)),
                    "masks": (f32, (T + 1, N, A, 1)), "active_masks": (f32, (T + 1, N, A, 1))}
    buf = DeviceRolloutBuffer(_HostEngine(cfg), T)
    for k in ("value_preds", "returns", "bad_masks", "available_actions", "advantages"):
        assert getattr(buf, k) is None
    assert buf._ws is None
    assert len(buf._carried()) == 6                              # obs, node_obs, adj, agent_id, masks, active_masks: nothing new is carried
    with pytest.raises(ValueError, match="value_preds"):
        buf.compute_returns(torch.zeros(N, A, 1))
    assert buf.available_actions_for(0) is None


def test_buffer_policy_fields_shapes_and_initial_values():
    from gmpe.rollout import DeviceRolloutBuffer, POLICY_FIELDS
    cfg = gmpe.make_config(num_envs=4, num_agents=3, episode_length=5)
    N, A, T, n = 4, 3, 6, cfg.n_actions
    buf = DeviceRolloutBuffer(_HostEngine(cfg), T, policy_fields="all")
    shapes = dict(value_preds=(T + 1, N, A, 1), returns=(T + 1, N, A, 1), bad_masks=(T + 1, N, A, 1), available_actions=(T + 1, N, A, n),
                  advantages=(T, N, A, 1))
    for k in POLICY_FIELDS:
        t = getattr(buf, k)
        assert tuple(t.shape) == shapes[k] and t.dtype == torch.float32
        assert float(t.min()) == float(t.max()) == (1.0 if k in ("bad_masks", "available_actions") else 0.0)   # graph_buffer.py:125-162
    assert buf._ws.numel() == gmpe.engine.returns_workspace_bytes(N * A)
    mine = torch.zeros(T + 1, N, A, 1)
    b2 = DeviceRolloutBuffer(_HostEngine(cfg), T, storage={"returns": mine})        # a storage entry requests its field
    assert b2.returns is mine and b2.value_preds is None
    with pytest.raises(ValueError, match="unknown policy"):
        DeviceRolloutBuffer(_HostEngine(cfg), T, policy_fields=("values",))
    with pytest.raises(ValueError, match="args"):
        DeviceRolloutBuffer(_HostEngine(cfg), T, policy_fields="all").compute_returns(torch.zeros(N, A, 1))


def _denorm(d, name):
    return None if name == "none" else (d[name + "_mean"].reshape(()), d[name + "_std"].reshape(()))


def test_numpy_restatement_is_the_reference_bit_for_bit():
    """tests/returns_lib.py against the vectors the reference produced (make_returns_fixture.py): returns, value_preds side effects and raw advantages
    bitwise, normalised advantages within float32 noise of np.nanmean / np.nanstd — every branch x {no normaliser, ValueNorm, PopArt}."""
    d = np.load(os.path.join(GOLD, "returns_advantages.npz"))
    for gae in (True, False):
        for proper in (False, True):
            for name in ("none", "valuenorm", "popart"):
                key = "%s_%s_%s" % ("gae" if gae else "mc", "proper" if proper else "plain", name)
                den = _denorm(d, name)
                ret, vp = R.np_returns(d["rewards"], d["masks"], d["value_preds"], d["returns_in"], d["next_value"], float(d["gamma"]),
                                       float(d["gae_lambda"]), gae, proper, d["bad_masks"], den)
                np.testing.assert_array_equal(ret.view(np.uint32), d["ret_" + key].view(np.uint32), err_msg=key)
                np.testing.assert_array_equal(vp.view(np.uint32), d["vp_" + key].view(np.uint32), err_msg=key)
                adv = R.np_advantages(ret, vp, den)
                np.testing.assert_array_equal(adv.view(np.uint32), d["adv_" + key].view(np.uint32), err_msg=key)
                np.testing.assert_allclose(R.np_normalized(adv, d["active_masks"]), d["advn_" + key], rtol=0, atol=1e-5, err_msg=key)


def test_numpy_stop_action_rule_is_the_reference():
    d = np.load(os.path.join(GOLD, "available_actions.npz"))
    T, n = int(d["T"]), int(d["n_actions"])
    for ep in range(d["dones"].shape[0]):
        np.testing.assert_array_equal(R.np_available_actions(d["dones"][ep], n), d["slots"][ep][1:])
        np.testing.assert_array_equal(d["policy_avail"][ep], d["slots"][ep][1:])          # what the policy acted with at step t sits in slot t + 1
    np.testing.assert_array_equal(d["slots"][1][0], d["slots"][0][T])                      # after_update carries the last slot
    assert (d["dones"].all(-1)).any() and (d["dones"].any(-1) & ~d["dones"].all(-1)).any()


# ------------------------------------------------------------------------------------------------ the advantage statistics: the inputs must discriminate
_V = R.VARIANTS
_ALWAYS = ("weight_b", "no_shortcuts", "ddof1", "inactive_kept", "last_wave_dropped")
_NINE = _ALWAYS + ("tail_dropped",)
# case -> the wrong variants of the kernel's order that leave the candidate set on it, (k_returns' order, k_advantages' order)
CAUGHT = {
    "offset": (("float32", "naive32") + _NINE, ("naive32",) + _NINE),            # float32 Welford happens to survive the ascending order ...
    "offset2": ((("float32", "naive32") + _NINE),) * 2,                          # ... of that seed, not of this one
    "unequal": (("float32", "naive32") + _NINE, ("float32",) + _NINE),
    "nan": (_NINE + ("nan_kept",),) * 2,
    "tail_partial": (("naive32",) + _NINE + ("hi_partials_dropped",),) * 2,      # T = 2: its only chunk is a tail
    "steps8": (_ALWAYS,) * 2,
    "steps9": (_NINE,) * 2,
    "steps16": (_ALWAYS,) * 2,
    "steps17": (_NINE,) * 2,
}
# where the float64 emulation of the kernel's order lands among the candidates: (dm, dd) in ulps, either order
HOST_OFFSETS = {k: (0, 0) for k in CAUGHT}
assert all(HOST_OFFSETS[k] == R.KERNEL_ORDER_OFFSETS for k in CAUGHT)            # what the GPU test holds the device to


def _candidate_cases():
    return [k for k in R.stat_cases() if k not in R.EXACT_CASES]


def test_statistics_cases_have_the_shapes_and_contents_they_claim():
    c = R.stat_cases()
    assert set(c) == set(CAUGHT) | set(R.EXACT_CASES)
    shapes = dict(offset=(9, 130), offset2=(9, 130), unequal=(9, 193), nan=(9, 130), tail_partial=(2, 64 * 257 + 5), const=(9, 130), two_equal=(3, 70),
                  **{"steps%d" % T: (T, 65) for T in (8, 9, 16, 17)})
    for k, (a, am) in c.items():
        assert a.shape == shapes[k] and am.shape == (a.shape[0] + 1, a.shape[1]), k
    a, am = c["offset"]
    m, s, n = R.stats64(a, am)
    assert abs(m - 100) < 0.1 and abs(s - 0.1) < 0.01 and 900 < np.hypot(m, s) / s < 1024
    m, s, n = R.stats64(*c["offset2"])
    assert abs(m - 100) < 0.1 and abs(s - 0.1) < 0.01 and 900 < np.hypot(m, s) / s < 1024
    a, am = c["unequal"]
    act = am[:9] != 0
    assert act[:, :64].all() and act[:, 64:128].sum() == 1 and a[:, 64:128][act[:, 64:128]] == 50 and not act[:, 128:192].any() and act[:, 192].all()
    a, am = c["nan"]
    act = am[:9] != 0
    assert np.isnan(a[act]).mean() >= 0.10 and np.isnan(a[~act]).any() and np.isposinf(a[~act]).any() and np.isneginf(a[~act]).any()
    assert (a[~act] == np.float32(1e30)).any() and (np.abs(a[~act]) < 100).any()
    a, am = c["tail_partial"]
    act = am[:2] != 0
    assert a.shape[1] > 257 * 64 and np.abs(a[:, :256 * 64][act[:, :256 * 64]]).max() < 0.2 and np.abs(a[:, 256 * 64:][act[:, 256 * 64:]] - 10).max() < 3
    assert act[:, 256 * 64:257 * 64].any() and act[:, 257 * 64:].any()
    a, am = c["const"]
    assert (a[am[:9] != 0] == R.CONST_VALUE).all() and (a[am[:9] == 0] != R.CONST_VALUE).all() and (am[:9] == 0).any()
    a, am = c["two_equal"]
    t, q = np.nonzero(am[:3])
    assert len(t) == 2 and q[0] // 64 != q[1] // 64 and a[t[0], q[0]] == a[t[1], q[1]]
    for k, (a, am) in c.items():                                                # a partial last wave and an inactive entry everywhere
        assert a.shape[1] % 64 and (am[:-1] == 0).any(), k


def test_stats64_and_candidates():
    rng = np.random.RandomState(0)
    a = (3 + rng.randn(5, 7, 1)).astype(np.float32)
    am = (rng.rand(6, 7, 1) > 0.3).astype(np.float32)
    a[1, 2] = np.nan
    x = a[:, :, 0][(am[:5, :, 0] != 0) & ~np.isnan(a[:, :, 0])].astype(np.float64)
    m, s, n = R.stats64(a, am)
    assert n == x.size and abs(m - x.mean()) < 1e-15 and abs(s - x.std()) < 1e-15
    assert R.stats64(a, np.zeros_like(am))[2] == 0
    pairs = R.candidate_pairs(m, s, n)
    assert len(pairs) == 15 and len({(p[2], p[3]) for p in pairs}) == 15
    one = np.float32(m)
    assert {p[2] for p in pairs} == {np.nextafter(one, np.float32(-9)), one, np.nextafter(one, np.float32(9))}
    d0 = np.float32(np.float32(s) + np.float32(1e-5))
    assert max(abs(float(p[3]) - float(d0)) for p in pairs) == 2 * float(np.spacing(d0))
    for bad in ((m, s, 1), (m, s, 2 ** 16 + 1), (m, 0.0, n), (2000.0, 1.0, n), (1e-4, 1.0, n), (0.0, 1.0, n)):
        with pytest.raises(AssertionError):
            R.candidate_pairs(*bad)
    # match_pair: the one candidate, NaN as NaN, None outside the set, and a constant input refused
    for dm, dd, mm, d in pairs:
        assert R.match_pair(a.view(np.uint32), R.normalize32(a, mm, d).view(np.uint32), pairs) == (dm, dd)
    far = R.normalize32(a, pairs[0][2], np.nextafter(pairs[0][3], np.float32(-9)))
    assert R.match_pair(a.view(np.uint32), far.view(np.uint32), pairs) is None
    c = np.full((4, 3), 2.5, np.float32)
    with pytest.raises(AssertionError, match="discriminate"):
        R.match_pair(c.view(np.uint32), R.normalize32(c, np.float32(2.5), d0).view(np.uint32), [(0, 0, np.float32(2.5), d0), (0, 1, np.float32(2.5), 2 * d0)])


@pytest.mark.parametrize("case", list(CAUGHT))
def test_kernel_order_lands_inside_and_every_wrong_variant_outside(case):
    """The float64 emulation of the kernel's order is inside the candidate set of every case, and the table of which wrong variant leaves it on
    which case is what CAUGHT says. Together the cases catch all ten."""
    a, am = R.stat_cases()[case]
    pairs = R.candidate_pairs(*R.stats64(a, am))
    for asc, want in zip((False, True), CAUGHT[case]):
        m, d = R.kernel_order_stats(a, am, asc)
        assert R.pair_offsets(m, d, pairs) == HOST_OFFSETS[case], (case, asc)
        # ... and the array it implies is told apart from every other candidate's
        assert R.match_pair(a.view(np.uint32), R.normalize32(a, m, d).view(np.uint32), pairs) == HOST_OFFSETS[case]
        caught = {v for v in _V if R.pair_offsets(*R.kernel_order_stats(a, am, asc, v), pairs) is None}
        assert caught == set(want), (case, asc, sorted(caught))


def test_every_wrong_variant_is_caught_by_a_named_case():
    for path in (0, 1):
        assert set(_V) == set().union(*(CAUGHT[k][path] for k in CAUGHT))
    assert [k for k in CAUGHT if "hi_partials_dropped" in CAUGHT[k][0]] == ["tail_partial"]
    assert [k for k in CAUGHT if "nan_kept" in CAUGHT[k][0]] == ["nan"]
    assert {k for k in CAUGHT if "tail_dropped" not in CAUGHT[k][0]} == {"steps8", "steps16"}     # no tail at a multiple of the unroll factor
    for path in (0, 1):                                                          # float32 accumulators: more than one case on either call site
        assert len([k for k in CAUGHT if "float32" in CAUGHT[k][path]]) >= 2


@pytest.mark.parametrize("T", R.STEP_TS)
def test_branch_inputs_stay_inside_the_candidate_limits(T):
    """The all-branches GPU test matches its normalised advantages to a candidate pair too: on the CPU, the advantages of every branch are inside
    candidate_pairs' limits (it asserts n and both condition numbers) and the kernel's order lands at the expected offsets in either order."""
    d = R.branch_inputs(T)
    for gae in (True, False):
        for proper in (False, True):
            for den in (None, R.DENORM):
                adv = R.branch_expectations(d, gae, proper, den)[2]
                pairs = R.candidate_pairs(*R.stats64(adv, d["active_masks"]))
                for asc in (False, True):
                    assert R.pair_offsets(*R.kernel_order_stats(adv, d["active_masks"], asc), pairs) == R.KERNEL_ORDER_OFFSETS, (T, gae, proper, asc)


@pytest.mark.parametrize("case", R.EXACT_CASES)
def test_constant_cases_are_exact_in_the_kernel_order(case):
    a, am = R.stat_cases()[case]
    m, s, n = R.stats64(a, am)
    assert m == float(R.CONST_VALUE) and s == 0.0 and n >= 2
    for asc in (False, True):
        assert R.kernel_order_stats(a, am, asc) == (R.CONST_VALUE, np.float32(1e-5))


def test_prescribed_inputs_give_the_prescribed_advantages():
    for case, (a, am) in R.stat_cases().items():
        T, L = a.shape
        p = R.prescribed_inputs(a, "advantages")
        assert R._same_bits(R.np_advantages(p["returns"], p["value_preds"]), a.reshape(T, L, 1)), case
        p = R.prescribed_inputs(a, "recurrence")
        with np.errstate(invalid="ignore"):
            ret, vp = R.np_returns(p["rewards"], p["masks"], p["value_preds"], p["returns"], p["next_value"], 0.99, 0.95, False, False)
            assert R._same_bits(R.np_advantages(ret, vp), a.reshape(T, L, 1)), case
