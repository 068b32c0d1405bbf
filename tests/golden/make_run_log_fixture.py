"""Golden vectors for gmpe.infos and gmpe.policy.eval_episode, produced by RUNNING the reference in this container:

    python tests/golden/make_run_log_fixture.py        # writes tests/golden/run_log.npz

What runs is the reference's own code, unbound on a namespace runner (ref_harness' and make_buffer_fixture's stubs; wandb.log records what log_env logs):
  * Runner.process_infos + Runner.log_env (onpolicy/runner/shared/base_runner.py:194-302) on prescribed info rows for N in {5, 130, 8200} x A = 3, handed
    over as the vec env builds them: per env a list of per-agent dicts of Python floats widened from float32. The rows hold full-mantissa values of
    mixed magnitudes and Time_req_to_goal values of exactly -1. The N = 5 case is built without 'Min_time_to_goal' (a world without max_speed). The
    runner carries `dt` = the world's dt: the reference never assigns `self.dt`.
  * GMPERunner.eval (onpolicy/runner/shared/graph_mpe_runner.py:445-516) on stub eval envs that replay prescribed rewards and dones over 6 steps (env 0
    finishes early, env 1 has one agent done from step 2 on, env 2 finishes on the last step) and a stub policy.act that records the masks and the RNN
    states it is handed and returns prescribed non-zero states. As shipped, eval assigns zeros of shape (k, recurrent_N, hidden) to the (k, A,
    recurrent_N, hidden) rows of the k finished envs (:495-499, and (k, 1) to (k, A, 1) masks, :503-505), which NumPy broadcasts only for k == 1 or
    k == A — with k == 0, any step at which no env finishes, it raises ValueError. So the prescribed dones finish exactly one env at every step
    (env 4 fills the steps at which no other env finishes) and A = 3 envs at step 3; what the code does there is what it means to do at any k.

Recorded (data only):
  infos/<N>/info            f32 [N, 3, 18]; for N = 8200 as infos/8200/pool f32 [256, 3, 18] and infos/8200/index i16 [8200]: info = pool[index]
  infos/<N>/names, values   what log_env logged, in its order: the keys and the float64 means
  infos/<N>/episode_length, dt, min_time
  eval/rewards f64 [6, 5, 3], eval/dones bool [6, 5, 3], eval/rnn_out f32 [6, 15, 1, 4] (what act returned)
  eval/masks_in f32 [6, 15, 1], eval/rnn_in f32 [6, 15, 1, 4] (what act was handed), eval/sums f64 [5, 3] and eval/mean (what log_env logged),
  eval/reward_dtype (of np.array(eval_episode_rewards))
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_buffer_fixture as MB  # noqa: E402

INFO_KEYS = ["individual_reward", "Dist_to_goal", "Time_req_to_goal", "Num_agent_collisions", "Num_obst_collisions", "Distance_mean",
             "Distance_variance", "Mean_by_variance", "Dists_traveled", "Time_taken", "Time_mean", "Time_stddev", "Time_mean_by_stddev",
             "Conformance", "Delta_spacing", "Spacing_violations", "Min_time_to_goal", "Phase_reached"]
A, T_INFOS, WORLD_DT = 3, 25, 0.1


def info_rows(rng, n):
    """float32 [n, A, 18]: full-mantissa values of mixed magnitudes, counts, and -1 in about a third of the Time_req_to_goal entries"""
    x = (rng.standard_normal((n, A, 18)) * np.exp(rng.uniform(-6.0, 6.0, (n, A, 18)))).astype(np.float32)
    x[..., 3] = rng.randint(0, 7, (n, A))
    x[..., 4] = rng.randint(0, 3, (n, A))
    ttg = np.abs(x[..., 2]) + np.float32(0.1)
    ttg[rng.rand(n, A) < 0.35] = -1.0
    x[..., 2] = ttg
    return x


def as_infos(info, min_time):
    keys = [(j, k) for j, k in enumerate(INFO_KEYS) if k != "Phase_reached" and (min_time or k != "Min_time_to_goal")]
    return [[{k: float(info[e, a, j]) for j, k in keys} for a in range(info.shape[1])] for e in range(info.shape[0])]


def run_infos(Runner, logged, info, min_time):
    runner = types.SimpleNamespace(num_agents=A, all_args=types.SimpleNamespace(episode_length=T_INFOS), dt=WORLD_DT)
    del logged[:]
    env_infos = Runner.process_infos(runner, as_infos(info, min_time))
    Runner.log_env(runner, env_infos, 100)
    assert all(step == 100 and len(d) == 1 for d, step in logged)
    names = [list(d)[0] for d, _ in logged]
    values = [list(d.values())[0] for d, _ in logged]
    assert all(isinstance(v, np.float64) for v in values)
    return names, np.array(values, dtype=np.float64)


class ReplayEvalEnvs(object):
    def __init__(self, rewards, dones, n_actions):
        self.rewards, self.dones, self.t = rewards, dones, 0
        self.action_space = [type("Discrete", (object,), {"n": n_actions})()]      # eval dispatches on the class name
        self.N, self.A = rewards.shape[1:]

    def _obs(self):
        z = np.zeros((self.N, self.A, 1))
        return z, z, z, z

    def reset(self):
        return self._obs()

    def step(self, actions_env):
        assert actions_env.shape == (self.N, self.A, self.action_space[0].n)
        t = self.t
        self.t += 1
        return self._obs() + (self.rewards[t].copy(), self.dones[t].copy(), [None] * self.N)


def run_eval(GMPERunner, Runner, logged):
    import torch
    rng = np.random.RandomState(7)
    T, N, R, H = 6, 5, 1, 4
    rewards = (rng.standard_normal((T, N, A)) * np.exp(rng.uniform(-4.0, 4.0, (T, N, A)))).astype(np.float32).astype(np.float64)
    dones = np.zeros((T, N, A), dtype=bool)
    dones[1, 0] = True                      # env 0 finishes early (and plays on after its auto-reset)
    dones[2:, 1, 1] = True                  # env 1: one agent done, never the env
    dones[T - 1, 2] = True                  # env 2 finishes on the last step
    dones[3, [0, 3]] = True                 # step 3: envs 0, 3 and 4 finish — A envs at once
    dones[[0, 2, 3, 4], 4] = True           # env 4 finishes wherever no other env does: see the module docstring
    assert all(int(dones[t].all(axis=1).sum()) in (1, A) for t in range(T))
    rnn_out = (rng.standard_normal((T, N * A, R, H)) + 3.0).astype(np.float32)          # non-zero: a zeroed row shows
    masks_in, rnn_in = [], []

    def act(obs, node_obs, adj, agent_id, rnn_states, masks, deterministic=False):
        assert deterministic is True
        masks_in.append(np.array(masks, dtype=np.float32).copy())
        rnn_in.append(np.array(rnn_states, dtype=np.float32).copy())
        t = len(masks_in) - 1
        return torch.zeros((N * A, 1), dtype=torch.int64), torch.from_numpy(rnn_out[t].copy())

    envs = ReplayEvalEnvs(rewards, dones, 5)
    runner = types.SimpleNamespace(eval_envs=envs, n_eval_rollout_threads=N, num_agents=A, episode_length=T, recurrent_N=R, hidden_size=H,
                                   buffer=types.SimpleNamespace(rnn_states=np.zeros((T + 1, N, A, R, H), dtype=np.float32)),
                                   trainer=types.SimpleNamespace(prep_rollout=lambda: None, policy=types.SimpleNamespace(act=act)))
    runner.log_env = types.MethodType(Runner.log_env, runner)
    del logged[:]
    GMPERunner.eval(runner, 200)
    assert len(logged) == 1 and logged[0][1] == 200 and list(logged[0][0]) == ["eval_average_episode_rewards"] and len(masks_in) == T
    mean = logged[0][0]["eval_average_episode_rewards"]
    stacked = np.array([rewards[t] for t in range(T)])          # eval's own expressions on the list it built from the same step() returns
    sums = np.sum(stacked, axis=0)
    assert isinstance(mean, np.float64) and np.mean(sums) == mean
    return dict(rewards=rewards, dones=dones, rnn_out=rnn_out, masks_in=np.array(masks_in), rnn_in=np.array(rnn_in), sums=sums, mean=np.float64(mean),
                reward_dtype=np.array(str(stacked.dtype)))


def main():
    _, GMPERunner = MB.load_reference()
    from onpolicy.runner.shared.base_runner import Runner
    logged = []
    sys.modules["wandb"].log = lambda d, step=None: logged.append((dict(d), step))
    out = {"info_keys": np.array(INFO_KEYS), "cases": np.array([5, 130, 8200])}
    rng = np.random.RandomState(20)
    for n in (5, 130, 8200):
        min_time = n != 5
        if n == 8200:
            pool = info_rows(rng, 256)
            index = rng.randint(0, 256, n).astype(np.int16)
            info = pool[index]
            out["infos/8200/pool"], out["infos/8200/index"] = pool, index
        else:
            info = info_rows(rng, n)
            out["infos/%d/info" % n] = info
        names, values = run_infos(Runner, logged, info, min_time)
        assert (info[..., 2] == -1).any() and len(names) == A * (16 + int(min_time)), (n, len(names))
        out["infos/%d/names" % n], out["infos/%d/values" % n] = np.array(names), values
        out["infos/%d/episode_length" % n], out["infos/%d/dt" % n], out["infos/%d/min_time" % n] = T_INFOS, WORLD_DT, min_time
        print("infos N = %d: %d keys logged, first %s = %r" % (n, len(names), names[0], values[0]))
    for k, v in run_eval(GMPERunner, Runner, logged).items():
        out["eval/" + k] = v
    print("eval: reward dtype %s, mean %r" % (out["eval/reward_dtype"], out["eval/mean"]))
    p = os.path.join(HERE, "run_log.npz")
    np.savez_compressed(p, **out)
    print(p, os.path.getsize(p))


if __name__ == "__main__":
    sys.exit(main())
