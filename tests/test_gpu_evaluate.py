"""Batched evaluator on the GPU (gmpe.evaluate, include/gmpe.h gmpe_episode_record / _metrics / _summary).

1. Reference pin: the reference's recorded rollouts (tests/golden/*_guided.npz) cut into the render loop's episodes, uploaded step by step into the
   engine's output tensors with the fixture env at several env indices and random distractors elsewhere; the records against the reference's own
   render loop (tests/golden/eval_metrics.npz) and every env against the NumPy restatement (tests/eval_lib.py), masks and stop rows every step.
2. Engine integration: 4096-env batches under seeded random actions; every step's outputs copied to the host and replayed through eval_lib.
3. Render-loop semantics: one-env engines (env_id_base = i) driven by the reference's loop shape on the host reproduce env i of the batch.
4. Repeatability: two evaluate() runs give bitwise equal summaries; record() past T raises.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import eval_lib as EL  # noqa: E402
import gmpe  # noqa: E402
import replay_lib as RL  # noqa: E402
from gmpe import evaluate as EV  # noqa: E402
from gmpe.engine import GmpeEngine  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden")
FIX = np.load(os.path.join(GOLDEN, "eval_metrics.npz"))
ROLLOUTS = [str(r) for r in FIX["rollouts"]]
DT, THRESH = float(FIX["dt"]), float(FIX["min_dist_thresh"])
EXACT = ["steps", "success", "collisions"]


def _compare_summary(summ, cols, A, label=""):
    ref = EL.summary_stats(cols, A)
    for c in EL.COLUMNS:
        got = summ["stats"][c]
        for k in ("min", "p10", "median", "p90", "max"):
            assert got[k] == ref[c][k] or (np.isnan(got[k]) and np.isnan(ref[c][k])), "%s %s %s: %r vs %r" % (label, c, k, got[k], ref[c][k])
        np.testing.assert_allclose([got["mean"], got["std"]], [ref[c]["mean"], ref[c]["std"]], rtol=1e-12, atol=1e-300, err_msg=label + c)


@pytest.mark.parametrize("name", ROLLOUTS)
def test_reference_pin_mixed_batch(name):
    path = os.path.join(GOLDEN, name + ".npz")
    d = np.load(path)
    A, T = int(d["A"]), int(d["episode_length"])
    segs = [tuple(s) for s in FIX[name + "/seg"]]
    N = 256
    eng = GmpeEngine(RL.fixture_config(d, path, N), 0)
    ev = EV.BatchedEvaluator(eng, episode_length=T, dt=DT, min_dist_thresh=THRESH)
    slots = RL.spread_slots(N, 4)
    W = d["info"].shape[-1]
    rng = np.random.RandomState(7)
    got_rows = []
    for ep, (s, n) in enumerate(segs):
        ev.reset()
        rec = EL.Record(N, A, T)
        for t in range(T):
            rew = rng.randn(N, A).astype(np.float32) * 3
            done = rng.rand(N, A) < 0.15
            info = (rng.rand(N, A, 18) * 4 - 1).astype(np.float32)
            info[..., 2] = np.where(rng.rand(N, A) < 0.5, -1.0, np.floor(info[..., 2] * 10))      # Time_req_to_goal: -1 or a step count
            if t < n:                                  # the fixture's episode; past its end its env is frozen and sees random rows
                rew[slots] = d["rew"][s + t].astype(np.float32)
                done[slots] = d["done"][s + t]
                info[slots] = 0.0
                info[slots, :, :W] = d["info"][s + t].astype(np.float32)
            eng.out.reward.copy_(torch.from_numpy(rew))
            eng.out.done.copy_(torch.from_numpy(done.astype(np.uint8)))
            eng.out.info.copy_(torch.from_numpy(info))
            ev.record()
            masks, avail = rec.step(rew, done, info)
            np.testing.assert_array_equal(ev.masks.cpu().numpy(), masks, err_msg="%s ep %d t=%d masks" % (name, ep, t))
            np.testing.assert_array_equal(ev.available_actions.cpu().numpy(), avail, err_msg="%s ep %d t=%d available_actions" % (name, ep, t))
        rows, cols = ev.episodes()
        assert cols == EL.COLUMNS
        rows = rows.cpu().numpy()
        np.testing.assert_array_equal(rows, EL.episode_columns(rec.final_info, rec.ret, rec.steps, T, DT, THRESH), err_msg="%s ep %d" % (name, ep))
        got_rows.append(rows[slots])
    ref = FIX[name + "/cols"]
    for k, sl in enumerate(slots):
        got = np.array([r[k] for r in got_rows])
        for j, c in enumerate(EL.COLUMNS):
            if c in EXACT:
                np.testing.assert_array_equal(got[:, j], ref[:, j], err_msg="%s slot %d %s" % (name, sl, c))
            else:
                np.testing.assert_allclose(got[:, j], ref[:, j], rtol=1e-5, atol=1e-5, err_msg="%s slot %d %s" % (name, sl, c))


BATCHES = [
    dict(scenario_name="nav_metered_one_goal_graph_rotate_tube_july", num_agents=10, episode_length=25, seed=11),
    dict(scenario_name="nav_graph_metered_single_corridor_rot_inv", num_agents=6, episode_length=30, seed=12),
    dict(scenario_name="navigation_graph", num_agents=8, num_obstacles=3, episode_length=25, seed=13),
]


@pytest.mark.parametrize("kw", BATCHES, ids=lambda k: "%s_A%d" % (k["scenario_name"][:12], k["num_agents"]))
def test_engine_integration_4096_envs(kw):
    N = 4096
    cfg = gmpe.make_config(num_envs=N, **kw)
    eng = GmpeEngine(cfg, 0)
    T, A = cfg.episode_length, cfg.num_agents
    R, H = 1, 8
    rnn = torch.zeros((N, A, R, H), dtype=torch.float32, device=eng.device)
    ev = EV.BatchedEvaluator(eng, rnn_states=rnn)
    assert ev.dt == cfg.dt and ev.T == T and ev.min_dist_thresh == EV.DEFAULT_MIN_DIST_THRESH
    ev.reset()
    rec = EL.Record(N, A, T, n_actions=cfg.n_actions)
    g = torch.Generator(device=eng.device).manual_seed(5)
    for t in range(T):
        a = torch.randint(0, cfg.n_actions, (N, A), generator=g, device=eng.device, dtype=torch.int32)
        o = eng.step(a)
        rnn.fill_(1.0)
        ev.record()
        masks, avail = rec.step(o.reward.cpu().numpy(), o.done.cpu().numpy().astype(bool), o.info.cpu().numpy())
        np.testing.assert_array_equal(ev.masks.cpu().numpy(), masks, err_msg="t=%d masks" % t)
        np.testing.assert_array_equal(ev.available_actions.cpu().numpy(), avail, err_msg="t=%d available_actions" % t)
        done = o.done.cpu().numpy().astype(bool)
        np.testing.assert_array_equal(rnn.cpu().numpy(), np.where(done[..., None, None], 0.0, 1.0).astype(np.float32).repeat(H, -1),
                                      err_msg="t=%d rnn rows" % t)
    with pytest.raises(RuntimeError, match="more than episode_length"):
        ev.record()
    rows, _ = ev.episodes()
    rows = rows.cpu().numpy()
    np.testing.assert_array_equal(ev.steps.cpu().numpy(), rec.steps)
    np.testing.assert_array_equal(ev.ret.cpu().numpy(), rec.ret)
    cols = EL.episode_columns(rec.final_info, rec.ret, rec.steps, T, cfg.dt, EV.DEFAULT_MIN_DIST_THRESH)
    np.testing.assert_array_equal(rows, cols)
    summ = ev.summary()
    _compare_summary(summ, rows, A)
    dists, times = EL.agent_sums(rec.final_info, T, cfg.dt)
    np.testing.assert_allclose(summ["dists_traveled"], dists, rtol=1e-12)
    np.testing.assert_allclose(summ["time_taken"], times, rtol=1e-12)
    assert summ["episodes"] == N and len(ev.csv_row()) == 5 + len(EV._CSV_STATS)
    eng.check_errors()


def _policy_np(obs, masks, n_actions):
    """Stand-in deterministic policy: a fixed function of obs, the stop action where the mask is 0."""
    a = (np.floor(np.abs(obs[..., 0]) * np.float32(1000.0)).astype(np.int64) + np.arange(obs.shape[1])) % n_actions
    return np.where(masks[..., 0] == 0, n_actions // 2, a).astype(np.int32)


def _policy_torch(obs, node_obs, adj, agent_id, masks, available_actions):
    n_actions = available_actions.shape[-1]
    a = (torch.floor(obs[..., 0].abs() * 1000.0).to(torch.int64) + torch.arange(obs.shape[1], device=obs.device)) % n_actions
    return torch.where(masks[..., 0] == 0, n_actions // 2, a).to(torch.int32)


def test_render_loop_semantics_per_env():
    kw = dict(scenario_name="nav_graph_metered_single_corridor_rot_inv", num_agents=4, episode_length=40, seed=21)
    N = 8
    eng = GmpeEngine(gmpe.make_config(num_envs=N, **kw), 0)
    ev = EV.BatchedEvaluator(eng)
    summ = EV.evaluate(eng, _policy_torch, evaluator=ev)
    ev_rows = ev.episodes()[0].cpu().numpy()
    T, A = 40, 4
    host_rows = []
    for i in range(N):
        one = GmpeEngine(gmpe.make_config(num_envs=1, env_id_base=i, **kw), 0)
        o = one.reset()
        masks = np.ones((1, A, 1), np.float32)
        ret = np.zeros((1, A))
        info = None
        for step in range(T):                                   # graph_mpe_runner.py:566-656, one env
            a = _policy_np(o.obs.cpu().numpy(), masks, one.cfg.n_actions)
            o = one.step(torch.from_numpy(a))
            ret = ret + o.reward.cpu().numpy().astype(np.float64)
            dones = o.done.cpu().numpy().astype(bool)
            info = o.info.cpu().numpy()
            masks = np.ones((1, A, 1), np.float32)
            masks[dones] = 0.0
            masks[dones.all(axis=1)] = 1.0
            if dones.all():
                break
        host_rows.append(EL.episode_columns(info, ret, np.array([step + 1]), T, one.cfg.dt, EV.DEFAULT_MIN_DIST_THRESH)[0])
        one.close()
    np.testing.assert_array_equal(ev_rows, np.array(host_rows))
    assert summ["stats"]["steps"]["max"] <= T


def test_repeatable_and_bounded():
    kw = dict(scenario_name="two_phase_graph", num_agents=5, episode_length=20, seed=31)
    eng = GmpeEngine(gmpe.make_config(num_envs=512, **kw), 0)

    def run():
        g = torch.Generator(device=eng.device).manual_seed(3)
        act = lambda obs, *rest: torch.randint(0, 25, obs.shape[:2], generator=g, device=obs.device, dtype=torch.int32)
        ev = EV.BatchedEvaluator(eng)
        s = EV.evaluate(eng, act, evaluator=ev)
        return s, ev.episodes()[0].cpu().numpy(), ev

    state = eng.get_state()                   # the same seed: the engine's RNG counters and state as before the first run
    s1, r1, ev = run()
    eng.set_state(state)
    s2, r2, _ = run()
    np.testing.assert_array_equal(r1, r2)
    for k in s1:
        if k == "stats":
            assert s1[k] == s2[k]
        else:
            np.testing.assert_array_equal(s1[k], s2[k], err_msg=k)
    with pytest.raises(RuntimeError, match="more than episode_length"):
        ev.record()
    ev.reset()
    with pytest.raises(RuntimeError, match="complete"):
        ev.episodes()
    s3 = EV.evaluate(eng, lambda obs, *rest: torch.zeros(obs.shape[:2], dtype=torch.int32, device=obs.device), stop_when_finished=5)
    assert s3["episodes"] == 512
    with pytest.raises(ValueError, match="with_info"):
        EV.BatchedEvaluator(GmpeEngine(gmpe.make_config(num_envs=4, **kw), 0, with_info=False))
