"""MultiDeviceGraphMPEVecEnv over real libgmpe handles == one BatchedGraphMPEVecEnv over the same N envs, bit for bit.

Repeated ordinals put several shards on one GPU: that runs the whole code path (split, env_id_base offsets, per-shard launches, D2H into row ranges of
the shared pinned arrays, sharded infos) on a one-GPU box. With two or more GPUs visible the July case also runs over devices [0, 1]."""
import argparse

import numpy as np
import pytest
import torch

from gmpe._lib import GmpeError
from gmpe.vec_env import BatchedGraphMPEVecEnv, MultiDeviceGraphMPEVecEnv, make_train_env

pytestmark = pytest.mark.gpu

JULY = "nav_metered_one_goal_graph_rotate_tube_july"


def _args(**over):
    d = dict(env_name="GraphMPE", scenario_name=JULY, dynamics_type="air_taxi", world_size=4, num_agents=10, num_landmarks=10, num_scripted_agents=0,
             num_obstacles=0, num_walls=0, collaborative=False, max_speed=2, collision_rew=5, formation_rew=1, goal_rew=5, episode_length=8,
             n_rollout_threads=64, total_actions=5, graph_feat_type="relative", discrete_action=True, use_safety_filter=False, seed=17)
    d.update(over)
    return argparse.Namespace(**d)


def _actions(rng, t, N, A, n_act):
    """Step t's actions in one of the forms a runner may pass: NumPy float64 one-hot, NumPy int64 indices, CUDA float32 one-hot, CUDA int indices."""
    idx = rng.randint(0, n_act, (N, A))
    form = t % 4
    if form == 0:
        return np.eye(n_act)[idx]
    if form == 1:
        return idx
    if form == 2:
        return torch.from_numpy(np.eye(n_act, dtype=np.float32)[idx]).to("cuda:0")
    return torch.from_numpy(idx).to("cuda:0", dtype=torch.int32 if t % 8 == 3 else torch.int64)


def _assert_same(got, ref, what):
    assert len(got) == len(ref), what
    for k, (g, r) in enumerate(zip(got, ref)):
        if k == 6:
            assert len(g) == len(r), what
            np.testing.assert_array_equal(g.as_array(), r.as_array(), err_msg="%s infos" % what)
            for e in (0, len(r) // 2, len(r) - 1):
                for dg, dr in zip(g[e], r[e]):
                    assert list(dg) == list(dr), (what, e)
                    np.testing.assert_array_equal(list(dg.values()), list(dr.values()), err_msg="%s infos[%d]" % (what, e))
        elif k == 7:
            assert g == r, (what, "reset_count")
        else:
            assert g.dtype == r.dtype and g.shape == r.shape, (what, k)
            np.testing.assert_array_equal(g, r, err_msg="%s output %d" % (what, k))


def _run_pair(args, N, devices, steps=30, **kw):
    multi = MultiDeviceGraphMPEVecEnv(args, devices, num_envs=N, **kw)
    ref = BatchedGraphMPEVecEnv(args, num_envs=N, device=0, **kw)
    try:
        _assert_same(multi.reset(), ref.reset(), "reset")
        rng = np.random.RandomState(5)
        n_act, dones = ref.action_space[0].n, 0
        for t in range(steps):
            a = _actions(rng, t, N, args.num_agents, n_act)
            r = ref.step(a, t)
            _assert_same(multi.step(a, t), r, "step %d" % t)
            dones += int(r[5].all(axis=1).sum())
        return dones
    finally:
        multi.close(); ref.close()


CASES = {
    "july_4096_x2": (dict(episode_length=8), 4096, [0, 0]),
    "nav_1000_x3": (dict(scenario_name="navigation_graph", dynamics_type="double_integrator", num_obstacles=3, num_walls=4, world_size=5), 1000, [0, 0, 0]),
    "rot_inv_x2": (dict(scenario_name="nav_graph_metered_single_corridor_rot_inv"), 600, [0, 0]),
    "two_phase_x2": (dict(scenario_name="two_phase_graph"), 600, [0, 0]),
    "three_phase_x2": (dict(scenario_name="three_phase_graph"), 600, [0, 0]),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_bit_identical_to_one_handle(case):
    over, N, devices = CASES[case]
    dones = _run_pair(_args(**over), N, devices)
    assert dones >= N                                        # auto-resets happened inside the 30 steps


def test_bit_identical_over_two_gpus():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs: this box exposes %d, so devices=[0, 1] cannot run (the repeated-ordinal cases cover the code path)"
                    % torch.cuda.device_count())
    torch.cuda.set_device(0)
    assert _run_pair(_args(), 4096, [0, 1]) >= 4096
    assert torch.cuda.current_device() == 0                  # the shards' C calls leave the caller's current device as it was


def test_unpinned_materialised_adjacency_and_rot_family_info_keys():
    over, N, devices = CASES["rot_inv_x2"]
    _run_pair(_args(**over), 300, devices, steps=10, pinned_host=False, adj_broadcast_view=False)
    env = make_train_env(_args(scenario_name="two_phase_graph", n_rollout_threads=10), devices=[0, 0])
    assert isinstance(env, MultiDeviceGraphMPEVecEnv)
    env.reset()
    infos = env.step(np.zeros((10, 10), dtype=np.int64))[6]
    assert len(infos) == 10 and len(infos[9][0]) == 18 and "Phase_reached" in infos[9][0] and infos.as_array().shape == (10, 10, 18)
    env.close()


def test_eval_surface_reset_count_sees_every_shard():
    """Shard 1's episodes are shifted by 3 steps (its current_step counters are set at reset, and the reference's rows the same way): reset_count is 1
    exactly at the steps where envs of shard 0 or of shard 1 reset, as the single handle's is."""
    N, L = 16, 6
    args = _args(n_rollout_threads=N, episode_length=L, num_agents=4, num_landmarks=4)
    multi = MultiDeviceGraphMPEVecEnv(args, [0, 0], eval_surface=True)
    ref = BatchedGraphMPEVecEnv(args, num_envs=N, eval_surface=True)
    _assert_same(multi.reset(), ref.reset(), "reset")
    lo = multi._shards[1].cfg.env_id_base
    multi._shards[1].engine.set("current_step", 3)
    cs = ref.engine.get("current_step"); cs[lo:] = 3
    ref.engine.set("current_step", cs)
    counts = []
    for t in range(13):
        a = np.zeros((N, 4), dtype=np.int64)
        out = multi.step(a)
        _assert_same(out, ref.step(a), "step %d" % t)
        assert out[7] == int(out[5].all(axis=1).any())
        counts.append(out[7])
    assert counts == [0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0]
    multi.close(); ref.close()


def test_hand_off_lifetimes():
    """Step t's arrays are intact after step t+1; step t's infos read after step t+2 raise."""
    env = MultiDeviceGraphMPEVecEnv(_args(n_rollout_threads=50), [0, 0, 0])
    env.reset()
    a = np.zeros((50, 10), dtype=np.int64)
    o1 = env.step(a)
    keep = [np.array(x) for x in o1[:6]]
    o2 = env.step(a + 3)
    for k, (x, y) in enumerate(zip(o1[:6], keep)):
        assert np.array_equal(x, y), k
    assert not np.array_equal(o2[0], keep[0])
    o2[6].as_array()
    i3 = env.step(a)[6]
    env.step(a); env.step(a)
    with pytest.raises(RuntimeError, match="overwrote"):
        i3[0]
    env.close()


def test_safety_filter_per_shard_equals_single_handle():
    """A filter that holds agent 0's controls at zero in every env: per shard == over the whole batch."""
    calls = []

    def hold_agent0(engine, actions_dev):
        n, A = engine.cfg.num_envs, engine.cfg.num_agents
        calls.append((engine.cfg.env_id_base, n, actions_dev.device))
        use = torch.zeros((n, A), dtype=torch.uint8, device=engine.device)
        use[:, 0] = 1
        return torch.zeros((n, A, 2), dtype=torch.float64, device=engine.device), use
    args = _args(n_rollout_threads=90, use_safety_filter=True)
    _run_pair(args, 90, [0, 0, 0], steps=12, safety_filter=hold_agent0)
    # every step: the single handle's one call over 90 envs, then one call per shard with that shard's envs
    assert [c[:2] for c in calls] == [(0, 90), (0, 30), (30, 30), (60, 30)] * 12
    assert all(c[2] == torch.device("cuda", 0) for c in calls)


def test_sticky_errors_name_their_shard():
    args = _args(world_size=0.5, num_agents=8, num_landmarks=8, n_rollout_threads=8)
    env = MultiDeviceGraphMPEVecEnv(args, [0, 0])
    with pytest.raises(GmpeError, match=r"shard 0 of 2 \(cuda:0, envs 0\.\.3\): reset placement gave up.*shard 1 of 2 \(cuda:0, envs 4\.\.7\)"):
        env.reset()
    env.close()
    assert env.closed
    env = MultiDeviceGraphMPEVecEnv(args, [0, 0])
    for s in env._shards:
        s.engine.reset()
    with pytest.raises(GmpeError, match="shard 1 of 2"):
        env.close()
    assert env.closed and all(s.closed for s in env._shards)
