"""MultiDeviceGraphMPEVecEnv on the CPU: the split / offset / hand-off / infos / error logic over shards whose engine is the CPU oracle.

The shards are the real BatchedGraphMPEVecEnv (upload, safety filter, info buffers, D2H issue, error checks) with an oracle-backed engine in place of
the HIP one — test infrastructure only; tests/test_gpu_multidevice_vec_env.py runs the same class over real handles and compares it with one handle
bit for bit."""
import argparse
import re

import numpy as np
import pytest
import torch

import gmpe
import oracle_lib as ol
from gmpe import vec_env
from gmpe._lib import GmpeError
from gmpe.config import INFO_KEYS
from gmpe.engine import GmpeEngine, StepOutputs
from gmpe.vec_env import BatchedGraphMPEVecEnv, MultiDeviceGraphMPEVecEnv

JULY = "nav_metered_one_goal_graph_rotate_tube_july"


def _args(**over):
    d = dict(env_name="GraphMPE", scenario_name=JULY, dynamics_type="air_taxi", world_size=4, num_agents=3, num_landmarks=3, num_scripted_agents=0,
             num_obstacles=0, num_walls=0, collaborative=False, max_speed=2, collision_rew=5, formation_rew=1, goal_rew=5, episode_length=4,
             n_rollout_threads=11, total_actions=5, graph_feat_type="relative", discrete_action=True, use_safety_filter=False, seed=21)
    d.update(over)
    return argparse.Namespace(**d)


def _nav_args(**over):
    kw = dict(scenario_name="navigation_graph", dynamics_type="double_integrator", num_obstacles=2, num_walls=4, world_size=3)
    kw.update(over)
    return _args(**kw)


class _OracleEngine(object):
    """GmpeEngine's surface as BatchedGraphMPEVecEnv uses it (out / rebind / reset / step / step_onehot / state_tensor / check_errors /
    set_control_override / close), computed by the CPU oracle into the bound CPU tensors."""

    def __init__(self, cfg, adj_compact):
        self.cfg, self.adj_compact, self.device = cfg, adj_compact, torch.device("cpu")
        N, A, E = cfg.num_envs, cfg.num_agents, cfg.num_entities
        self.N, self.A = N, A
        self.orc = ol.Oracle(cfg)
        self.out = StepOutputs(obs=torch.zeros(N, A, cfg.obs_dim), agent_id=torch.zeros(N, A, 1, dtype=torch.int32),
                               node_obs=torch.zeros(N, A, E, cfg.node_feats), adj=torch.zeros((N, E, E) if adj_compact else (N, A, E, E)),
                               reward=torch.zeros(N, A), done=torch.zeros(N, A, dtype=torch.uint8), info=torch.zeros(N, A, len(INFO_KEYS)))
        self._err = torch.zeros(N, dtype=torch.int32)
        self.h = True

    def rebind(self, o):
        for k in StepOutputs.__slots__:
            a, b = getattr(self.out, k), getattr(o, k)
            assert (a is None) == (b is None) and (a is None or (a.shape == b.shape and a.dtype == b.dtype and b.is_contiguous())), k
        self.out = o

    def _fill(self, obs, ids, node, adj):
        o = self.out
        o.obs.copy_(torch.from_numpy(obs)); o.agent_id.copy_(torch.from_numpy(ids)); o.node_obs.copy_(torch.from_numpy(node))
        o.adj.copy_(torch.from_numpy(adj if self.adj_compact else np.broadcast_to(adj[:, None], o.adj.shape)))
        self._err.copy_(torch.from_numpy(self.orc.get("error_flags")))

    def reset(self):
        self._fill(*self.orc.reset())
        return self.out

    def step(self, act):
        assert act.dtype == torch.int32 and tuple(act.shape) == (self.N, self.A)
        obs, ids, node, adj, rew, done, info, _ = self.orc.step(act.numpy())
        self._fill(obs, ids, node, adj)
        o = self.out
        o.reward.copy_(torch.from_numpy(rew)); o.done.copy_(torch.from_numpy(done.astype(np.uint8))); o.info.copy_(torch.from_numpy(info))
        return o

    def step_onehot(self, onehot):
        assert onehot.dtype == torch.float32 and tuple(onehot.shape) == (self.N, self.A, self.cfg.n_actions)
        return self.step(onehot.argmax(dim=-1).to(torch.int32))

    def state_tensor(self, name):
        assert name == "error_flags"
        return self._err

    def get(self, name):
        return self.orc.get(name)

    check_errors = GmpeEngine.check_errors

    def set_control_override(self, ctrl=None, use=None):
        self.orc.set_control_override(None if ctrl is None else ctrl.numpy(), None if use is None else use.numpy())

    def close(self):
        self.h = False


class _OracleShard(BatchedGraphMPEVecEnv):
    def _make_engine(self, cfg, device):
        return _OracleEngine(cfg, self._compact)

    @staticmethod
    def _empty_host(shape, dtype, pinned):
        return torch.empty(tuple(shape), dtype=dtype)          # no pinned memory without a GPU; the two-set hand-off is the same

    def _sync(self):
        pass


class _CpuMulti(MultiDeviceGraphMPEVecEnv):
    """world_of_last: a world size for the last shard only (a too-small world there)."""
    world_of_last = None

    def _make_shard(self, device, **kw):
        args = self._all_args
        if self.world_of_last is not None and kw["env_id_base"] == self._ranges[-1][0]:
            args = argparse.Namespace(**dict(vars(args), world_size=self.world_of_last))
        return _OracleShard(args, device=device, **kw)


class _SmallLastWorld(_CpuMulti):
    world_of_last = 0.5


def _oracle(args, N):
    return ol.Oracle(gmpe.config_from_args(args, num_envs=N))


def test_split_tables_and_refusals():
    for N, devs, sizes in ((1000, [0, 0, 0], [334, 333, 333]), (5, [0, 0, 0, 0], [2, 1, 1, 1]), (4096, [0] * 8, [512] * 8)):
        env = _CpuMulti(_args(n_rollout_threads=N), devs)
        assert env.num_envs == N and [s.num_envs for s in env._shards] == sizes
        assert [s.cfg.env_id_base for s in env._shards] == [sum(sizes[:g]) for g in range(len(sizes))]
        assert [s.cfg.num_envs for s in env._shards] == sizes and sum(sizes) == N
        env.close()
        assert all(s.closed for s in env._shards)
    with pytest.raises(ValueError, match="6 shards for 5 envs"):
        _CpuMulti(_args(n_rollout_threads=5), [0] * 6)
    with pytest.raises(ValueError, match="at least one device"):
        _CpuMulti(_args(), [])
    for make in (vec_env.make_train_env, vec_env.make_eval_env):
        for dev in (0, 1):
            with pytest.raises(ValueError, match="not both"):
                make(_args(), device=dev, devices=[0, 0])


def _expect(ref, env):
    """ref: the N-env oracle's outputs (float64) as the float32 / int32 / bool arrays the engine hands over."""
    f32 = lambda x: np.asarray(x).astype(np.float32)
    out = [f32(ref[0]), ref[1], f32(ref[2]), np.broadcast_to(f32(ref[3])[:, None], (env.num_envs, env.num_agents) + ref[3].shape[1:])]
    if len(ref) > 4:
        out += [f32(ref[4]), ref[5]]
    return out


@pytest.mark.parametrize("scen", ["navigation_graph", "july"])
@pytest.mark.parametrize("form", ["onehot", "index", "index_tensor"])
def test_twelve_steps_equal_one_oracle_run(scen, form):
    """Three uneven shards (4 / 4 / 3 envs) through step() with auto-resets == one 11-env oracle run: every returned array and infos.as_array()."""
    args = _nav_args() if scen == "navigation_graph" else _args()
    N = args.n_rollout_threads
    env = _CpuMulti(args, [0, 0, 0])
    assert [s.num_envs for s in env._shards] == [4, 4, 3]
    orc = _oracle(args, N)
    got, ref = env.reset(), orc.reset()
    for k, (g, r) in enumerate(zip(got, _expect(ref, env))):
        np.testing.assert_array_equal(g, r, err_msg="reset out %d" % k)
    rng = np.random.RandomState(3)
    n_act = env.action_space[0].n
    resets, prev, prev_copy = 0, None, None
    for t in range(12):
        idx = rng.randint(0, n_act, (N, env.num_agents))
        acts = {"onehot": np.eye(n_act)[idx], "index": idx, "index_tensor": torch.from_numpy(idx)}[form]
        out = env.step(acts, t)
        ref = orc.step(idx)
        assert len(out) == 7 and out[5].dtype == bool and out[3].shape == (N, env.num_agents) + ref[3].shape[1:]
        for k, (g, r) in enumerate(zip(out[:6], _expect(ref, env))):
            np.testing.assert_array_equal(g, r, err_msg="t=%d out %d" % (t, k))
        infos = out[6]
        assert len(infos) == N and len(infos[N - 1]) == env.num_agents
        np.testing.assert_array_equal(infos.as_array(), ref[6].astype(np.float32).astype(np.float64))
        assert infos[N - 1][2]["Dist_to_goal"] == float(np.float32(ref[6][N - 1, 2, 1]))
        if prev is not None:                                     # step t-1's arrays are untouched by step t
            for k, (a, b) in enumerate(zip(prev, prev_copy)):
                np.testing.assert_array_equal(a, b, err_msg="t=%d out %d of the step before" % (t, k))
        prev, prev_copy = out[:6], [np.array(x) for x in out[:6]]
        resets += int(ref[7].sum())
    assert resets >= 2 * N
    keys = set(out[6][0][0])
    assert len(keys) == 17 and "Phase_reached" not in keys
    env.close()


def test_unpinned_eval_surface_and_stale_infos():
    args = _args(n_rollout_threads=7)
    env = _CpuMulti(args, [0, 1], pinned_host=False, eval_surface=True)
    orc = _oracle(args, 7)
    env.reset(); orc.reset()
    rng = np.random.RandomState(4)
    counts, outs, infos = [], [], []
    for t in range(9):
        idx = rng.randint(0, 25, (7, 3))
        out = env.step(idx)
        ref = orc.step(idx)
        assert len(out) == 8
        np.testing.assert_array_equal(out[0], ref[0].astype(np.float32))
        assert out[7] == int(ref[5].all(axis=1).any())
        counts.append(out[7])
        outs.append(out[0]); infos.append(out[6])
    assert counts == [0, 0, 0, 1, 0, 0, 0, 1, 0]
    assert all(a is not b and not np.shares_memory(a, b) for a, b in zip(outs, outs[1:]))     # fresh arrays every step
    infos[-2].as_array()                                         # read one step late: fine
    with pytest.raises(RuntimeError, match="overwrote"):
        infos[-3][0]
    env.close()


def test_safety_filter_sees_one_shard_at_a_time():
    """f(shard_engine, shard_actions_dev) once per shard and step; the overridden controls give the N-env oracle's run with the same override."""
    args = _args(n_rollout_threads=9)
    seen = []

    def brake(engine, actions_dev):
        n = engine.cfg.num_envs
        seen.append((engine.cfg.env_id_base, n, tuple(actions_dev.shape)))
        ctrl = torch.zeros((n, engine.cfg.num_agents, 2), dtype=torch.float64)
        use = torch.zeros((n, engine.cfg.num_agents), dtype=torch.uint8)
        use[:, 0] = 1
        return ctrl, use

    env = _CpuMulti(args, [0, 0, 0], safety_filter=brake)
    orc = _oracle(args, 9)
    ctrl = np.zeros((9, 3, 2)); use = np.zeros((9, 3), np.uint8); use[:, 0] = 1
    orc.set_control_override(ctrl, use)
    env.reset(); orc.reset()
    rng = np.random.RandomState(6)
    for t in range(5):
        idx = rng.randint(0, 25, (9, 3))
        out = env.step(np.eye(25)[idx])
        ref = orc.step(idx)
        np.testing.assert_array_equal(out[0], ref[0].astype(np.float32))
        np.testing.assert_array_equal(out[2], ref[2].astype(np.float32))
    assert seen[:3] == [(0, 3, (3, 3, 25)), (3, 3, (3, 3, 25)), (6, 3, (3, 3, 25))] and len(seen) == 15
    env.close()


def test_too_small_world_in_the_last_shard_raises_naming_it():
    args = _args(n_rollout_threads=10, num_agents=8, num_landmarks=8)
    named = "shard 2 of 3 (cuda:0, envs 7..9): reset placement gave up"

    make = lambda: _SmallLastWorld(args, [0, 0, 0])
    env = make()
    with pytest.raises(GmpeError, match="^" + re.escape(named)) as ei:
        env.reset()
    assert "shard 0" not in str(ei.value) and "shard 1" not in str(ei.value)
    env.close()                                                   # reported by reset(): not raised again
    assert env.closed and all(s.closed for s in env._shards)
    env2 = make()
    for s in env2._shards:
        s.engine.reset()                                          # engine-level reset: nobody has looked at the flags
    with pytest.raises(GmpeError, match=re.escape(named)):
        env2.step(np.zeros((10, 8), dtype=np.int64))
    env2.close()
    assert env2.closed
    env3 = make()
    for s in env3._shards:
        s.engine.reset()
    with pytest.raises(GmpeError, match=re.escape(named)):
        env3.close()                                              # the last hand-off raises them, once, after closing every shard
    assert env3.closed and all(s.closed and not s.engine.h for s in env3._shards)
    env3.close()


def test_factories_pick_the_class(monkeypatch):
    made = []
    monkeypatch.setattr(vec_env, "BatchedGraphMPEVecEnv", lambda a, **kw: made.append(("single", kw)) or "single")
    monkeypatch.setattr(vec_env, "MultiDeviceGraphMPEVecEnv", lambda a, devices, **kw: made.append(("multi", devices, kw)) or "multi")
    a = _args(n_rollout_threads=8, n_eval_rollout_threads=1)
    assert vec_env.make_train_env(a) == "single" and made[-1] == ("single", dict(num_envs=8, device=0, eval_surface=False))
    assert vec_env.make_train_env(a, device=1, eval_surface=True) == "single" and made[-1][1]["device"] == 1
    assert vec_env.make_train_env(a, devices=[3]) == "single" and made[-1][1]["device"] == 3
    assert vec_env.make_train_env(a, devices=[0, 1]) == "multi" and made[-1] == ("multi", [0, 1], dict(num_envs=8, eval_surface=False))
    assert vec_env.make_train_env(a, devices=(0, 0, 0), eval_surface=True) == "multi" and made[-1][2]["eval_surface"]
    assert vec_env.make_eval_env(a) == "single" and made[-1] == ("single", dict(num_envs=1, device=0, eval_surface=True))
    a.n_eval_rollout_threads = 4
    assert vec_env.make_eval_env(a, devices=[0, 1]) == "multi" and made[-1] == ("multi", [0, 1], dict(num_envs=4, eval_surface=False))
    assert vec_env.make_eval_env(a, devices=[2]) == "single" and made[-1][1]["device"] == 2
