"""CPU side of the series evaluator (include/gmpe.h gmpe_episode_record_series, gmpe.evaluate episodes_per_env / merge): the plan's layout
against the C header, the exported symbol, the argument checks of the C entry point and of the Python layer (refused before any device call), the
NumPy restatement (tests/eval_series_lib.py) against six cheap wrong variants on the test inputs, and the engine-driven scenarios' shares of early
and time-limit episode ends on the CPU oracle."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import abi_lib  # noqa: E402
import eval_lib as EL  # noqa: E402
import eval_series_lib as SL  # noqa: E402
import gmpe  # noqa: E402
from gmpe import _lib  # noqa: E402
from gmpe import evaluate as EV  # noqa: E402
from gmpe.engine import GmpeEngine  # noqa: E402

FIELDS = ["num_envs", "num_agents", "num_steps", "num_episodes", "n_actions", "rnn_row", "reward", "done", "info", "episode", "t_in_ep", "ret",
          "steps", "ret_out", "final_info", "masks", "available_actions", "rnn_states"]


def test_symbol_is_exported_and_bound():
    assert "gmpe_episode_record_series" in _lib.SYMBOLS and "gmpe_episode_record_series" in abi_lib.exported()
    assert _lib.load().gmpe_abi_version() == 3 and gmpe.config.ABI_VERSION == 3  # an added entry point: the ABI version stays


def test_plan_layout_matches_the_c_header():
    P = _lib.GmpeEpisodeSeriesPlan
    assert [f for f, _ in P._fields_] == FIELDS
    size, fields = abi_lib.layout(P)
    assert (size, fields) == abi_lib.mirror_layout(P) and size == 6 * 4 + 12 * 8
    # the existing record plan is untouched
    size, fields = abi_lib.layout(_lib.GmpeEpisodeRecordPlan)
    assert size == 6 * 4 + 10 * 8 and fields["reward"][0] == 24 and fields["rnn_states"][0] == 24 + 9 * 8


FAKE = 0x1000      # an aligned non-null address: every plan below is refused before it could be used


def _plan(**kw):
    p = _lib.GmpeEpisodeSeriesPlan()
    p.num_envs, p.num_agents, p.num_steps, p.num_episodes, p.n_actions = 8, 3, 5, 2, 25
    for f in FIELDS[6:-1]:
        setattr(p, f, FAKE)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("plan, msg", [
    (_plan(num_episodes=0), "num_episodes >= 1"),
    (_plan(num_episodes=-3), "num_episodes >= 1"),
    (_plan(num_episodes=1 << 20, num_envs=1 << 11), "2^31 - 1"),
    (_plan(num_episodes=2, num_envs=1 << 30), "2^31 - 1"),
    (_plan(num_steps=0), "num_steps >= 1"),
    (_plan(num_envs=0), "num_envs >= 1"),
    (_plan(num_agents=65), "num_agents <= 64"),
    (_plan(n_actions=0), "n_actions"),
    (_plan(n_actions=4097), "n_actions"),
    (_plan(reward=None), "null pointer"),
    (_plan(episode=None), "null pointer"),
    (_plan(t_in_ep=None), "null pointer"),
    (_plan(ret_out=None), "null pointer"),
    (_plan(final_info=None), "null pointer"),
    (_plan(masks=None), "null pointer"),
    (_plan(rnn_states=FAKE, rnn_row=0), "rnn_row"),
    (_plan(ret=FAKE + 4), "misaligned"),
    (_plan(ret_out=FAKE + 4), "misaligned"),
    (_plan(t_in_ep=FAKE + 2), "misaligned"),
])
def test_c_side_refuses_bad_plans_before_any_device_call(plan, msg):
    lib = _lib.load()
    assert lib.gmpe_episode_record_series(0, C.byref(plan), None) == -1                   # GMPE_ERR_INVALID_ARG
    err = lib.gmpe_last_error()
    assert err.startswith(b"gmpe_episode_record_series: ") and msg.encode() in err, err


def test_c_side_null_plan_and_largest_accepted_row_count():
    lib = _lib.load()
    assert lib.gmpe_episode_record_series(0, None, None) == -1 and b"null plan" in lib.gmpe_last_error()
    # R * N = 2^31 - 1 passes the row check: the next check (a null pointer) is the one that refuses it
    assert lib.gmpe_episode_record_series(0, C.byref(_plan(num_episodes=1, num_envs=2 ** 31 - 1, masks=None)), None) == -1
    assert b"null pointer" in lib.gmpe_last_error()


def _stub_engine(N=8, A=3, T=25):
    """A GmpeEngine without a device handle: what the evaluator's constructor reads before it allocates anything."""
    eng = GmpeEngine.__new__(GmpeEngine)
    eng.h = C.c_void_p()
    eng.cfg = gmpe.make_config(num_envs=N, num_agents=A, episode_length=T)
    eng.N, eng.A, eng.device = N, A, None
    eng.out = types.SimpleNamespace(info=object())
    return eng


def test_python_layer_refuses_bad_series_arguments():
    with pytest.raises(ValueError, match="episodes_per_env must be >= 1"):
        EV.BatchedEvaluator(_stub_engine(), episodes_per_env=0)
    with pytest.raises(ValueError, match="episodes_per_env must be >= 1"):
        EV.BatchedEvaluator(_stub_engine(), episodes_per_env=-2)
    with pytest.raises(ValueError, match="2\\^31 - 1"):
        EV.BatchedEvaluator(_stub_engine(N=1 << 16), episodes_per_env=1 << 15)
    with pytest.raises(ValueError, match="engine's episode_length = 25"):
        EV.BatchedEvaluator(_stub_engine(T=25), episodes_per_env=2, episode_length=20)
    with pytest.raises(ValueError, match="engine's episode_length = 25"):
        EV.BatchedEvaluator(_stub_engine(T=25), types.SimpleNamespace(episode_length=30), episodes_per_env=3)


def _stub_evaluator(A=3, T=25, dt=1.0, thr=0.05, R=2, N=8, t=None):
    """A BatchedEvaluator as merge() sees it before it touches a tensor; t: calls recorded (default: all R * T, so finished)."""
    ev = EV.BatchedEvaluator.__new__(EV.BatchedEvaluator)
    ev.A, ev.T, ev.dt, ev.min_dist_thresh, ev.R, ev.N = A, T, dt, thr, R, N
    ev._t, ev._finished = R * T if t is None else t, False
    return ev


@pytest.mark.parametrize("kw, name", [(dict(A=4), "num_agents"), (dict(T=20), "episode_length"), (dict(dt=0.1), "dt"), (dict(thr=0.1), "min_dist_thresh"),
                                      (dict(R=3), "episodes_per_env")])
def test_merge_refuses_mismatched_evaluators(kw, name):
    with pytest.raises(ValueError, match="evaluator 1 has %s" % name):
        EV.merge([_stub_evaluator(), _stub_evaluator(**kw)])


def test_merge_refuses_unfinished_none_and_foreign_objects():
    never_reset = _stub_evaluator()
    never_reset._t = None
    with pytest.raises(RuntimeError, match="evaluator 1 is not finished"):
        EV.merge([_stub_evaluator(), never_reset])
    with pytest.raises(ValueError, match="at least one"):
        EV.merge([])
    with pytest.raises(TypeError, match="BatchedEvaluator"):
        EV.merge([object()])
    with pytest.raises(TypeError, match="MultiDeviceGraphMPEVecEnv"):
        EV.shard_evaluators(object())


# --- the restatement and its inputs

SHARP = dict(N=17, A=5, T=5, R=3, seed=3)


def _sharp_inputs():
    return SL.series_inputs(SHARP["N"], SHARP["A"], SHARP["T"], SHARP["R"], SHARP["seed"])


def test_restatement_by_hand():
    """Two envs, two agents, T = 3, R = 2: env 0 ends its first episode at its second step by all-done, then runs to the time limit; env 1 never
    reaches all-done: two time limits."""
    rew = np.arange(1, 13, dtype=np.float32).reshape(6, 2, 1).repeat(2, axis=2)            # call s: env 0 gets 2s + 1, env 1 gets 2s + 2
    done = np.zeros((6, 2, 2), bool)
    done[1, 0] = True
    done[2, 1, 0] = True
    info = np.arange(6 * 2 * 2 * 18, dtype=np.float32).reshape(6, 2, 2, 18)
    rec = SL.Series(2, 2, 3, 2, n_actions=5)
    states = []
    for s in range(6):
        masks, avail = rec.step(rew[s], done[s], info[s])
        states.append((rec.episode.tolist(), rec.t_in_ep.tolist()))
        if s == 2:
            np.testing.assert_array_equal(masks[..., 0], [[1, 1], [0, 1]])
            np.testing.assert_array_equal(avail[1, 0], [0, 0, 1, 0, 0])
        if s == 1:
            assert (masks == 1).all() and (avail == 1).all()                                # the all-done env acts next with ones
    assert states == [([0, 0], [1, 1]), ([1, 0], [0, 2]), ([1, 1], [1, 0]), ([1, 1], [2, 1]), ([2, 1], [0, 2]), ([2, 2], [0, 0])]
    np.testing.assert_array_equal(rec.steps, [[2, 3], [3, 3]])
    np.testing.assert_array_equal(rec.ret_out[:, :, 0], [[1 + 3, 2 + 4 + 6], [5 + 7 + 9, 8 + 10 + 12]])
    np.testing.assert_array_equal(rec.final_info[0, 0], info[1, 0])
    np.testing.assert_array_equal(rec.final_info[1, 0], info[4, 0])
    np.testing.assert_array_equal(rec.final_info[0, 1], info[2, 1])
    np.testing.assert_array_equal(rec.final_info[1, 1], info[5, 1])
    assert rec.finished() and (rec.ret == 0).all()


def test_one_episode_per_env_is_the_existing_record():
    N, A, T = 33, 5, 25
    rew, done, info = EL.record_inputs(N, A, T, seed=4)
    old, new = EL.Record(N, A, T), SL.Series(N, A, T, 1)
    for t in range(T):
        m0, a0 = old.step(rew[t], done[t], info[t])
        m1, a1 = new.step(rew[t], done[t], info[t])
        np.testing.assert_array_equal(m0, m1)
        np.testing.assert_array_equal(a0, a1)
        np.testing.assert_array_equal(old.live, new.episode == 0)
    np.testing.assert_array_equal(old.steps, new.steps[0])
    np.testing.assert_array_equal(old.ret, new.ret_out[0])
    np.testing.assert_array_equal(old.final_info.view(np.int32), new.final_info[0].view(np.int32))


def test_inputs_hold_the_patterns_the_kernel_must_meet():
    rew, done, info = _sharp_inputs()
    N, T, R = SHARP["N"], SHARP["T"], SHARP["R"]
    rec, trace = SL.replay(rew, done, info, T, R)
    assert rec.finished()
    assert ((rec.steps == 1).all(axis=0)).any()                            # an env whose every episode ends at its first step
    all_done = done.all(axis=2)
    never = [n for n in range(N) if (rec.steps[:, n] == T).all() and not all_done[:, n].any()]
    assert never                                                           # an env that meets the time limit only
    finish_call = np.array([next(s for s, tr in enumerate(trace) if tr["episode"][n] == R) for n in range(N)])
    assert len(set(finish_call.tolist())) >= 4 and finish_call.min() == R - 1 and finish_call.max() == R * T - 1
    frozen_all_done = [(s, n) for n in range(N) for s in range(finish_call[n] + 1, R * T) if all_done[s, n]]
    assert frozen_all_done                                                 # all-done rows reach envs that are frozen
    limits = [(s, n) for s, tr in enumerate(trace) for n in range(N)
              if tr["t_in_ep"][n] == 0 and not all_done[s, n] and (s == 0 or trace[s - 1]["episode"][n] < tr["episode"][n])]
    assert any((s + 1) % T for s, n in limits)                             # a time limit that does not fall on a multiple of T calls
    bits = info.view(np.int32)
    assert (bits == 0x7fc00000).any() and (bits == -4079307).any() and (bits == -2 ** 31).any()
    fb = rec.final_info.view(np.int32)
    assert (fb == 0x7fc00000).any() and (fb == -4079307).any() and (fb == -2 ** 31).any()          # and they reach the recorded rows


@pytest.mark.parametrize("variant", SL.VARIANTS)
def test_inputs_tell_the_restatement_from_wrong_variants(variant):
    rew, done, info = _sharp_inputs()
    good, gtrace = SL.replay(rew, done, info, SHARP["T"], SHARP["R"])
    bad, btrace = SL.replay(rew, done, info, SHARP["T"], SHARP["R"], variant=variant)
    g, b = good.arrays(), bad.arrays()
    differ = [k for k in ("steps", "ret_out", "final_info") if not np.array_equal(g[k], b[k])]
    per_call = [k for k in ("episode", "t_in_ep", "ret") if any(not np.array_equal(x[k], y[k]) for x, y in zip(gtrace, btrace))]
    assert differ or per_call, variant
    expect = {"ret not cleared": "ret_out", "terminal reward to the next episode": "ret_out", "env-major rows": "steps", "any-done ends": "steps",
              "global time limit": "steps", "records past R": "episode"}[variant]
    assert expect in differ + per_call, (variant, differ, per_call)


@pytest.mark.parametrize("case", SL.series_cases()[:36:5])
def test_direct_cases_finish_every_env_within_r_times_t_calls(case):
    N, A, R, T, na, row = case
    rew, done, info = SL.series_inputs(N, A, T, R, seed=N + A + R + T)
    assert rew.shape == (R * T, N, A) and done.dtype == bool and info.shape == (R * T, N, A, 18)
    rec, _ = SL.replay(rew, done, info, T, R, n_actions=na)
    assert rec.finished() and (rec.steps >= 1).all() and (rec.steps <= T).all()


def test_case_list_covers_the_issue_grid():
    cases = SL.series_cases()
    assert {(n, a) for n, a, *_ in cases} >= {(1, 1), (17, 64), (4099, 10)}
    assert {c[2] for c in cases} == {1, 2, 3, 7} and {c[3] for c in cases} == {1, 2, 25}
    assert {c[4] for c in cases} == {1, 2, 24, 25} and {c[5] for c in cases} == {None, 1, 7, 64, 1025}
    for N, A in SL.SERIES_SHAPES:
        mine = [c for c in cases if c[:2] == (N, A)]
        assert {c[4] for c in mine} == {1, 2, 24, 25} and len({c[5] for c in mine}) >= 4, (N, A)


# --- the engine-driven scenarios on the CPU oracle

def oracle_series(name):
    """The scenario under seek_actions on the CPU oracle until every env has played ENGINE_EPISODES episodes -> (Series, calls)."""
    import oracle_lib as ol
    cfg = gmpe.make_config(num_envs=SL.ENGINE_ENVS, **SL.ENGINE_SCENARIOS[name])
    orc = ol.Oracle(cfg)
    obs = orc.reset()[0]
    T, R = cfg.episode_length, SL.ENGINE_EPISODES
    rec = SL.Series(cfg.num_envs, cfg.num_agents, T, R, n_actions=cfg.n_actions)
    while not rec.finished():
        before = rec.episode.copy()
        out = orc.step(SL.seek_actions(obs, cfg.n_actions))
        obs = out[0]
        rec.step(out[4].astype(np.float32), out[5], out[6].astype(np.float32))
        ended = rec.episode > before
        np.testing.assert_array_equal(out[7][before < R], ended[before < R])        # an episode ends exactly where the oracle resets the env
        assert (orc.get("current_step")[ended] == 0).all()
    orc.close()
    return rec, rec.calls


@pytest.mark.parametrize("name", sorted(SL.ENGINE_SCENARIOS))
def test_engine_scenarios_end_both_ways_on_the_oracle(name):
    rec, calls = oracle_series(name)
    T = SL.ENGINE_SCENARIOS[name]["episode_length"]
    early, late = SL.end_shares(rec.steps, T)
    print("%s: %d episodes, %.3f end before T, %.3f at T, %d calls" % (name, rec.steps.size, early, late, calls))
    assert early >= 0.10 and late >= 0.10, (early, late)
    assert calls <= SL.ENGINE_EPISODES * T
