"""Several evaluation episodes per env and merged evaluators on the GPU (include/gmpe.h gmpe_episode_record_series, gmpe.evaluate
episodes_per_env / merge / shard_evaluators). References and inputs: tests/eval_series_lib.py (proven sharp on the CPU in
tests/test_eval_series_host.py) and the metric references of tests/eval_lib.py.

1. Direct: the entry point on synthetic tensors, every state and policy input against the NumPy restatement after every call, the records at the end.
2. R = 1: the same sequences through gmpe_episode_record and the series entry point, identical after every step.
3. Engine-driven: a tube scenario and navigation_graph under a deterministic goal seeker, three episodes per env; the record, episodes() and
   summary() against the restatement, both kinds of episode end present, the engine's current_step 0 after every recorded end.
4. Merge: one evaluator per shard of a two-shard env against one evaluator over all the envs, bit for bit.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import eval_lib as EL  # noqa: E402
import eval_series_lib as SL  # noqa: E402
import gmpe  # noqa: E402
from gmpe import _lib  # noqa: E402
from gmpe import evaluate as EV  # noqa: E402
from gmpe.engine import GmpeEngine  # noqa: E402
from gmpe.vec_env import BatchedGraphMPEVecEnv, MultiDeviceGraphMPEVecEnv, make_train_env  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 0


def _dev(a):
    return torch.from_numpy(np.array(a)).to("cuda:%d" % DEV)


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _ramp(shape, device):
    """A sentinel that is neither 0 nor 1 and differs from row to row: a write to the wrong row shows."""
    n = int(np.prod(shape))
    return (torch.arange(n, device=device, dtype=torch.int64) % 8191 + 2).to(torch.float32).reshape(shape)


def _same(t, a):
    """torch.equal of a device tensor and a NumPy array (NaN-free)."""
    return torch.equal(t.cpu(), torch.from_numpy(np.ascontiguousarray(a)))


class _SeriesState(object):
    """The tensors and the plan of one direct run of gmpe_episode_record_series."""

    def __init__(self, N, A, R, T, na, rnn_row):
        dev = torch.device("cuda:%d" % DEV)
        self.episode = torch.zeros((N,), dtype=torch.int32, device=dev)
        self.t_in_ep = torch.zeros((N,), dtype=torch.int32, device=dev)
        self.ret = torch.zeros((N, A), dtype=torch.float64, device=dev)
        self.steps = torch.full((R, N), -7, dtype=torch.int32, device=dev)
        self.ret_out = torch.full((R, N, A), -7.0, dtype=torch.float64, device=dev)
        self.final = torch.full((R, N, A, _lib.EVAL_INFO_WIDTH), -7.0, dtype=torch.float32, device=dev)
        self.masks = torch.full((N, A, 1), -7.0, dtype=torch.float32, device=dev)
        self.avail = torch.full((N, A, na), -7.0, dtype=torch.float32, device=dev)
        self.rnn = self.ramp = None
        if rnn_row is not None:
            self.ramp = _ramp((N, A, rnn_row), dev)
            self.rnn = torch.empty_like(self.ramp)
        p = self.plan = _lib.GmpeEpisodeSeriesPlan()
        p.num_envs, p.num_agents, p.num_steps, p.num_episodes, p.n_actions = N, A, T, R, na
        p.episode, p.t_in_ep, p.ret = self.episode.data_ptr(), self.t_in_ep.data_ptr(), self.ret.data_ptr()
        p.steps, p.ret_out, p.final_info = self.steps.data_ptr(), self.ret_out.data_ptr(), self.final.data_ptr()
        p.masks, p.available_actions = self.masks.data_ptr(), self.avail.data_ptr()
        if self.rnn is not None:
            p.rnn_states, p.rnn_row = self.rnn.data_ptr(), rnn_row

    def call(self, rew, done, info):
        self._in = (_dev(rew), _dev(done.astype(np.uint8)), _dev(info))
        if self.rnn is not None:
            self.rnn.copy_(self.ramp)
        p = self.plan
        p.reward, p.done, p.info = (x.data_ptr() for x in self._in)
        _lib.check(_lib.load().gmpe_episode_record_series(DEV, C.byref(p), _stream()), "gmpe_episode_record_series")

    def rnn_ok(self):
        want = torch.where(self._in[1].bool()[..., None], torch.zeros((), device=self.ramp.device), self.ramp)
        return torch.equal(self.rnn, want)


@pytest.mark.parametrize("N,A,R,T,na,rnn_row", SL.series_cases())
def test_series_direct(N, A, R, T, na, rnn_row):
    rew, done, info = SL.series_inputs(N, A, T, R, seed=N + A + R + T)
    st = _SeriesState(N, A, R, T, na, rnn_row)
    rec = SL.Series(N, A, T, R, n_actions=na)
    label = "N=%d A=%d R=%d T=%d n_actions=%d rnn_row=%r" % (N, A, R, T, na, rnn_row)
    finish_calls = set()
    for s in range(R * T):
        was = rec.episode.copy()
        st.call(rew[s], done[s], info[s])
        m, av = rec.step(rew[s], done[s], info[s])
        assert _same(st.episode, rec.episode), "%s call %d episode" % (label, s)
        assert _same(st.t_in_ep, rec.t_in_ep), "%s call %d t_in_ep" % (label, s)
        assert _same(st.ret, rec.ret), "%s call %d ret" % (label, s)
        np.testing.assert_array_equal(st.masks.cpu().numpy(), m, err_msg="%s call %d masks" % (label, s))
        np.testing.assert_array_equal(st.avail.cpu().numpy(), av, err_msg="%s call %d available_actions" % (label, s))
        if rnn_row is not None:
            assert st.rnn_ok(), "%s call %d rnn rows" % (label, s)
        if ((rec.episode == R) & (was < R)).any():
            finish_calls.add(s)
    assert rec.finished()
    if N >= 15 and T > 1:
        assert len(finish_calls) >= min(3, R * T), finish_calls        # envs finish at different calls and sit frozen while others run
    assert (rec.steps >= 1).all()                                      # every -7 of the outputs below has been overwritten
    assert _same(st.steps, rec.steps), label + " steps"
    assert _same(st.ret_out, rec.ret_out), label + " ret_out"
    np.testing.assert_array_equal(st.final.cpu().numpy().view(np.int32), rec.final_info.view(np.int32), err_msg=label + " final_info bits")


@pytest.mark.parametrize("N,A,na,rnn_row,T", [(1, 1, 1, None, 1), (17, 64, 24, 7, 2), (33, 5, 25, 64, 25), (4099, 10, 25, 1, 25), (1000, 3, 2, 1025, 25)])
def test_one_episode_per_env_equals_gmpe_episode_record(N, A, na, rnn_row, T):
    rew, done, info = EL.record_inputs(N, A, T, seed=N + T)
    st = _SeriesState(N, A, 1, T, na, rnn_row)
    dev = st.episode.device
    live = torch.ones((N,), dtype=torch.uint8, device=dev)
    steps = torch.full((N,), -7, dtype=torch.int32, device=dev)
    ret = torch.zeros((N, A), dtype=torch.float64, device=dev)
    final = torch.full((N, A, _lib.EVAL_INFO_WIDTH), -7.0, dtype=torch.float32, device=dev)
    masks = torch.full((N, A, 1), -7.0, dtype=torch.float32, device=dev)
    avail = torch.full((N, A, na), -7.0, dtype=torch.float32, device=dev)
    rnn = None if rnn_row is None else torch.empty_like(st.ramp)
    rp = _lib.GmpeEpisodeRecordPlan()
    rp.num_envs, rp.num_agents, rp.num_steps, rp.n_actions = N, A, T, na
    rp.live, rp.steps, rp.ret, rp.final_info = live.data_ptr(), steps.data_ptr(), ret.data_ptr(), final.data_ptr()
    rp.masks, rp.available_actions = masks.data_ptr(), avail.data_ptr()
    if rnn is not None:
        rp.rnn_states, rp.rnn_row = rnn.data_ptr(), rnn_row
    for t in range(T):
        st.call(rew[t], done[t], info[t])
        if rnn is not None:
            rnn.copy_(st.ramp)
        rp.t = t
        rp.reward, rp.done, rp.info = (x.data_ptr() for x in st._in)
        _lib.check(_lib.load().gmpe_episode_record(DEV, C.byref(rp), _stream()), "gmpe_episode_record")
        lv = live.bool()
        assert torch.equal(lv, st.episode == 0), t
        assert torch.equal(torch.where(lv, st.t_in_ep, st.steps[0]), torch.where(lv, torch.full_like(steps, t + 1), steps)), t
        assert torch.equal(torch.where(lv[:, None], st.ret, st.ret_out[0]), ret), t          # the running returns, then the recorded ones
        fin = ~lv
        assert torch.equal(st.final[0][fin].view(torch.int32), final[fin].view(torch.int32)), t
        assert torch.equal(st.masks, masks) and torch.equal(st.avail, avail), t
        if rnn is not None:
            assert torch.equal(st.rnn, rnn), t
    assert not live.any() and torch.equal(st.steps[0], steps) and torch.equal(st.ret_out[0], ret)
    assert torch.equal(st.final[0].view(torch.int32), final.view(torch.int32))


def _compare_summary(summ, cols, A, label=""):
    ref = EL.summary_stats(cols, A)
    for c in EL.COLUMNS:
        got = summ["stats"][c]
        for k in ("min", "p10", "median", "p90", "max"):
            assert got[k] == ref[c][k] or (np.isnan(got[k]) and np.isnan(ref[c][k])), "%s %s %s: %r vs %r" % (label, c, k, got[k], ref[c][k])
        np.testing.assert_allclose([got["mean"], got["std"]], [ref[c]["mean"], ref[c]["std"]], rtol=1e-12, atol=1e-300, err_msg=label + c)


@pytest.mark.parametrize("name", sorted(SL.ENGINE_SCENARIOS))
def test_engine_driven_three_episodes_per_env(name):
    """The scenarios of eval_series_lib.ENGINE_SCENARIOS (32 envs, 3 agents, T = 40) under seek_actions, R = 3. On the CPU oracle alone
    (tests/test_eval_series_host.py) the 96 episodes split as: tube_july 0.323 end before T and 0.677 at T; navigation_graph 0.417 before T and
    0.583 at T (120 calls each: some env plays three full-length episodes)."""
    cfg = gmpe.make_config(num_envs=SL.ENGINE_ENVS, **SL.ENGINE_SCENARIOS[name])
    N, A, T, R = cfg.num_envs, cfg.num_agents, cfg.episode_length, SL.ENGINE_EPISODES
    eng = GmpeEngine(cfg, DEV)
    H = 8
    rnn = torch.zeros((N, A, 1, H), dtype=torch.float32, device=eng.device)
    ev = EV.BatchedEvaluator(eng, rnn_states=rnn, episodes_per_env=R)
    assert ev.R == R and ev.T == T and tuple(ev.steps.shape) == (R, N) and tuple(ev.final_info.shape) == (R, N, A, 18)
    with pytest.raises(RuntimeError, match="before reset"):
        ev.record()
    o = ev.reset()
    rec = SL.Series(N, A, T, R, n_actions=cfg.n_actions)
    while not rec.finished():
        with pytest.raises(RuntimeError, match="complete"):
            ev.episodes()
        o = eng.step(torch.from_numpy(SL.seek_actions(o.obs.cpu().numpy(), cfg.n_actions)))
        rnn.fill_(1.0)
        ev.record()
        before = rec.episode.copy()
        done = o.done.cpu().numpy().astype(bool)
        masks, avail = rec.step(o.reward.cpu().numpy(), done, o.info.cpu().numpy())
        s = rec.calls
        np.testing.assert_array_equal(ev.masks.cpu().numpy(), masks, err_msg="call %d masks" % s)
        np.testing.assert_array_equal(ev.available_actions.cpu().numpy(), avail, err_msg="call %d available_actions" % s)
        np.testing.assert_array_equal(rnn.cpu().numpy(), np.where(done[..., None, None], 0.0, 1.0).astype(np.float32).repeat(H, -1),
                                      err_msg="call %d rnn rows" % s)
        assert _same(ev.episode, rec.episode) and _same(ev.t_in_ep, rec.t_in_ep) and _same(ev.ret_running, rec.ret), s
        ended = rec.episode > before
        assert (eng.get("current_step")[ended] == 0).all(), s             # an episode is recorded as over exactly where the engine reset the env
        assert ev.finished() == rec.finished()
    assert ev.t == rec.calls <= R * T
    assert _same(ev.steps, rec.steps) and _same(ev.ret, rec.ret_out)
    np.testing.assert_array_equal(ev.final_info.cpu().numpy().view(np.int32), rec.final_info.view(np.int32))
    early, late = SL.end_shares(rec.steps, T)
    print("%s: %.3f of %d episodes end before T, %.3f at T, %d calls" % (name, early, R * N, late, rec.calls))
    assert early >= 0.10 and late >= 0.10, (early, late)
    rows, names = ev.episodes()
    assert names == EL.COLUMNS and tuple(rows.shape) == (R * N, 16)
    rows = rows.cpu().numpy()
    cols = EL.episode_columns(rec.final_info.reshape(R * N, A, -1), rec.ret_out.reshape(R * N, A), rec.steps.reshape(-1), T, cfg.dt,
                              EV.DEFAULT_MIN_DIST_THRESH)
    np.testing.assert_array_equal(rows, cols)
    summ = ev.summary()
    _compare_summary(summ, rows, A, name + " ")
    dists, times = EL.agent_sums(rec.final_info.reshape(R * N, A, -1), T, cfg.dt)
    np.testing.assert_allclose(summ["dists_traveled"], dists, rtol=1e-12)
    np.testing.assert_allclose(summ["time_taken"], times, rtol=1e-12)
    assert summ["episodes"] == R * N
    row = ev.csv_row()
    assert len(row) == 5 + len(EV._CSV_STATS) and row[4] == R * N
    eng.check_errors()


def _policy(obs, node_obs, adj, agent_id, masks, available_actions):
    """A fixed function of obs, the stop action where the mask is 0."""
    n_actions = available_actions.shape[-1]
    a = (torch.floor(obs[..., 0].abs() * 1000.0).to(torch.int64) + torch.arange(obs.shape[1], device=obs.device)) % n_actions
    return torch.where(masks[..., 0] == 0, n_actions // 2, a).to(torch.int32)


def test_evaluate_runs_the_series_and_record_is_bounded():
    kw = dict(scenario_name="two_phase_graph", num_agents=5, episode_length=12, seed=31)
    eng = GmpeEngine(gmpe.make_config(num_envs=300, **kw), DEV)
    state = eng.get_state()
    ev = EV.BatchedEvaluator(eng, episodes_per_env=4)
    s1 = EV.evaluate(eng, _policy, evaluator=ev)
    assert ev.t == 48 and s1["episodes"] == 1200
    with pytest.raises(RuntimeError, match="more than episodes_per_env \\* episode_length = 48"):
        ev.record()
    r1 = ev.episodes()[0].clone()
    eng.set_state(state)
    s2 = EV.evaluate(eng, _policy, episodes_per_env=4, stop_when_finished=1)          # the same episodes, stopped once every env has its four
    np.testing.assert_array_equal(np.array([s1[lab] for lab, _, _ in EV.SUMMARY_LABELS]), np.array([s2[lab] for lab, _, _ in EV.SUMMARY_LABELS]))
    np.testing.assert_array_equal(s1["dists_traveled"].view(np.int64), s2["dists_traveled"].view(np.int64))
    assert r1.shape == (1200, 16)
    with pytest.raises(ValueError, match="engine's episode_length = 12"):
        EV.BatchedEvaluator(eng, episodes_per_env=2, episode_length=10)
    one = EV.BatchedEvaluator(eng, episode_length=10)                                   # one episode per env keeps its own episode_length
    assert one.R == 1 and one.T == 10 and tuple(one.steps.shape) == (300,) and isinstance(one._rec, _lib.GmpeEpisodeRecordPlan)


# --- merge

JULY = "nav_metered_one_goal_graph_rotate_tube_july"


def _args(**over):
    d = dict(env_name="GraphMPE", scenario_name=JULY, dynamics_type="air_taxi", world_size=4, num_agents=10, num_landmarks=10, num_scripted_agents=0,
             num_obstacles=0, num_walls=0, collaborative=False, max_speed=2, collision_rew=5, formation_rew=1, goal_rew=5, episode_length=8,
             n_rollout_threads=51, total_actions=5, graph_feat_type="relative", discrete_action=True, use_safety_filter=False, seed=17)
    d.update(over)
    return argparse.Namespace(**d)


def _play(evaluators):
    """Every evaluator's engine under _policy until all have finished."""
    outs = [ev.reset() for ev in evaluators]
    for _ in range(evaluators[0].R * evaluators[0].T):
        for g, ev in enumerate(evaluators):
            o = outs[g]
            outs[g] = ev.engine.step(_policy(o.obs, o.node_obs, o.adj, o.agent_id, ev.masks, ev.available_actions))
            ev.record()
        if all(ev.finished() for ev in evaluators):
            break


def _values(summ):
    return np.array([summ[lab] for lab, _, _ in EV.SUMMARY_LABELS] + [summ["stats"][c][k] for c in EV.COLUMNS for k in EV.STATS])


def _merge_case(args, devices, R):
    env = make_train_env(args, devices=devices)
    ref = BatchedGraphMPEVecEnv(args, num_envs=args.n_rollout_threads, device=devices[0])
    try:
        assert isinstance(env, MultiDeviceGraphMPEVecEnv)
        shards = EV.shard_evaluators(env, args, episodes_per_env=R)
        assert [ev.N for ev in shards] == [26, 25] and [ev.device.index for ev in shards] == devices
        single = EV.BatchedEvaluator(ref.engine, args, episodes_per_env=R)
        _play(shards)
        _play([single])
        merged = EV.merge(shards)
        N, A = args.n_rollout_threads, args.num_agents
        assert merged.N == N and merged.R == R and tuple(merged.final_info.shape) == (R, N, A, 18)
        rows, names = merged.episodes()
        ref_rows, ref_names = single.episodes()
        ref_rows = ref_rows.to(rows.device)
        assert names == ref_names and torch.equal(rows, ref_rows) and torch.equal(rows.view(torch.int64), ref_rows.view(torch.int64))
        assert torch.equal(merged.steps.cpu(), single.steps.reshape(R, N).cpu())
        sm, ss = merged.summary(), single.summary()
        assert sorted(sm) == sorted(ss) and sm["episodes"] == ss["episodes"] == R * N
        np.testing.assert_array_equal(_values(sm), _values(ss))
        for k in ("dists_traveled", "time_taken"):
            np.testing.assert_array_equal(sm[k].view(np.int64), ss[k].view(np.int64), err_msg=k)          # the fixed-tree sums, as bits
        rm, rs = merged.csv_row(args), single.csv_row(args)
        assert len(rm) == len(rs)
        for x, y in zip(rm, rs):
            np.testing.assert_array_equal(np.asarray(x), np.asarray(y))
        # the order matters: merged the other way round, the rows are another permutation of the same episodes
        swapped = EV.merge(shards[::-1]).episodes()[0]
        assert not torch.equal(swapped, rows) and torch.equal(swapped.view(torch.int64).sort(dim=0).values, rows.view(torch.int64).sort(dim=0).values)
        if R > 1:
            half = EV.BatchedEvaluator(ref.engine, args, episodes_per_env=R)
            half.reset()
            half.engine.step(torch.zeros((N, A), dtype=torch.int32, device=half.device))
            half.record()
            with pytest.raises(RuntimeError, match="not finished"):
                EV.merge([single, half])
            with pytest.raises(ValueError, match="episodes_per_env"):
                EV.merge([single, EV.BatchedEvaluator(ref.engine, args)])
    finally:
        env.close(); ref.close()


@pytest.mark.parametrize("R", [1, 2])
def test_merge_of_two_shards_equals_one_engine(R):
    _merge_case(_args(), [0, 0], R)


@pytest.mark.parametrize("R", [1, 2])
def test_merge_of_two_shards_equals_one_engine_navigation_graph(R):
    _merge_case(_args(scenario_name="navigation_graph", dynamics_type="double_integrator", num_agents=4, num_landmarks=4, num_obstacles=3,
                      world_size=2, episode_length=20), [0, 0], R)


def test_merge_over_two_gpus():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs: this box exposes %d, so devices=[0, 1] cannot run (the repeated-ordinal cases cover the code path)"
                    % torch.cuda.device_count())
    torch.cuda.set_device(0)
    _merge_case(_args(), [0, 1], 2)
