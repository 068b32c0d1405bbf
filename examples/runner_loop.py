"""The reference runner's collect loop (onpolicy/runner/shared/graph_mpe_runner.py:57-103) over the batched engine, three ways, and a fourth
with the action head inside the loop:

  (1) drop-in: `BatchedGraphMPEVecEnv` in place of `GraphSubprocVecEnv` — NumPy in, NumPy out, the runner unchanged;
  (2) device-resident, open loop: `DeviceRolloutBuffer.collect` — ONE launch writes the whole `[T+1, N, A, ...]` rollout in HBM,
      and the GNN's edge list (`process_adj`, onpolicy/algorithms/utils/gnn_new.py:329-358) is built on the device;
  (3) device-resident, policy in the loop: the policy reads slot `step` of the buffer as device tensors and `insert_step` writes slot `step + 1`
      in place, the policy's outputs (values, actions, log-probs, RNN states) included — the runner change of INTEGRATION.md §7 (no NumPy one-hot up,
      no seven arrays down per step), followed by returns, PPO minibatches and after_update on the device;
  (4) as (3), with the action head in the launch sequence: the policy stops at its logits and `act_step` masks them from the previous step's dones, draws
      the action on the engine's Philox stream, writes action and log-prob into the buffer slots and steps the env (one launch instead of the
      Categorical's torch ops); the stored log-probs are bit for bit what `gmpe.ppo_losses` recomputes.

The policy is a stand-in (uniform random actions): the learner is outside this package's scope.

    python examples/runner_loop.py --envs 4096 --agents 10 --episodes 3
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gmpe  # noqa: E402


def reference_args(n_envs, n_agents, episode_length, scenario):
    """The fields `GraphMPEEnv(args)` reads (multiagent/MPE_env.py:56-84), as the reference's train script sets them."""
    return argparse.Namespace(
        env_name="GraphMPE", scenario_name=scenario, dynamics_type="air_taxi", world_size=4, num_agents=n_agents, num_landmarks=n_agents,
        num_scripted_agents=0, num_obstacles=0, num_walls=0, collaborative=False, max_speed=2, collision_rew=5, formation_rew=1, goal_rew=5,
        use_dones=False, episode_length=episode_length, num_env_steps=10 ** 6, n_rollout_threads=n_envs, render_episodes=None, fair_wt=1,
        fair_rew=1, formation_type="point", total_actions=5, zeroshift=5, graph_feat_type="relative", discrete_action=True,
        use_safety_filter=False, seed=1)


def drop_in_loop(args, episodes):
    from gmpe.vec_env import make_train_env
    envs = make_train_env(args)
    N, A, n_act = envs.num_envs, args.num_agents, envs.action_space[0].n
    rng = np.random.RandomState(0)
    obs, agent_id, node_obs, adj = envs.reset()                                  # GMPERunner.warmup, :213-238
    eye = np.eye(n_act)
    t0, ret = time.perf_counter(), 0.0
    for ep in range(episodes):
        for step in range(args.episode_length):
            actions_env = eye[rng.randint(0, n_act, (N, A))]                     # the runner's one-hot (:375-377)
            obs, agent_id, node_obs, adj, rewards, dones, infos = envs.step(actions_env)
            ret += float(rewards.mean())
    dt = time.perf_counter() - t0
    sample = infos[0][0]                                                         # built lazily, only when read (base_runner.py:194-290)
    envs.close()
    return dict(path="drop-in (NumPy boundary)", env_steps_per_s=N * episodes * args.episode_length / dt, mean_step_reward=ret / (episodes * args.episode_length),
                shapes=dict(obs=obs.shape, node_obs=node_obs.shape, adj=adj.shape), info_keys=len(sample))


def device_loop(args, episodes, max_edge_dist=1.0):
    import torch
    from gmpe.engine import GmpeEngine
    from gmpe.rollout import DeviceRolloutBuffer
    from gmpe.config import config_from_args
    cfg = config_from_args(args)
    eng = GmpeEngine(cfg, adj_compact=True)                                      # one [N,E,E] matrix per env; buf.adj is the broadcast view
    buf = DeviceRolloutBuffer(eng, args.episode_length)
    buf.warmup()
    g = torch.Generator(device=eng.device); g.manual_seed(0)
    T, N, A = args.episode_length, cfg.num_envs, cfg.num_agents
    torch.cuda.synchronize(); t0 = time.perf_counter()
    n_edges = 0
    for ep in range(episodes):
        actions = torch.randint(0, cfg.n_actions, (T, N, A), generator=g, device=eng.device, dtype=torch.int32)
        buf.collect(actions)                                                     # T steps, ONE launch, every slot written in place
        ei, ew, m = eng.edges_from_adj_compact(buf._adj[T], A, max_edge_dist)    # the learner's int64 edge set for the last slot's N*A graphs
        n_edges = int(m)
        buf.after_update()
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    return dict(path="device-resident rollout buffer", env_steps_per_s=N * episodes * T / dt, mean_step_reward=float(buf.rewards.mean()),
                shapes=dict(obs=tuple(buf.obs.shape), node_obs=tuple(buf.node_obs.shape), adj=tuple(buf.adj.shape)), edges_last_slot=n_edges,
                masks_zero=int((buf.masks == 0).sum()))


def device_closed_loop(args, episodes, hidden_size=16):
    """Policy in the loop without leaving the GPU: GMPERunner.collect's inputs are slot `step` of the device buffer, the policy's outputs
    (values, int64 actions, log-probs, RNN states) go straight into `insert_step`, which writes every learner field in one launch after the env step; then
    compute_returns -> the PPO generators -> after_update, with no learner-owned array outside the buffer. The stand-in policy is a linear layer on `obs` and a
    tanh recurrence (the learner is out of scope); what matters is the data flow."""
    import torch
    from gmpe.engine import GmpeEngine
    from gmpe.rollout import DeviceRolloutBuffer
    from gmpe.config import config_from_args
    cfg = config_from_args(args)
    eng = GmpeEngine(cfg, adj_compact=True)
    run_args = argparse.Namespace(gamma=0.99, gae_lambda=0.95, use_gae=True, use_proper_time_limits=False, use_valuenorm=False, use_popart=False,
                                  recurrent_N=1, hidden_size=hidden_size)
    buf = DeviceRolloutBuffer(eng, args.episode_length, policy_fields="all", learner_fields="all", args=run_args)
    buf.warmup()                                                                 # GMPERunner.warmup, :213-238
    T, N, A = args.episode_length, cfg.num_envs, cfg.num_agents
    torch.manual_seed(0)
    head = torch.nn.Linear(cfg.obs_dim + hidden_size, cfg.n_actions + 1 + hidden_size).to(eng.device)
    n_mb = 0
    torch.cuda.synchronize(); t0 = time.perf_counter()
    with torch.no_grad():
        for ep in range(episodes):
            for step in range(T):
                h = buf.rnn_states[step].flatten(0, 1)                           # [N*A, 1, H]: zeroed for agents done at step - 1, carried by after_update
                out = head(torch.cat([buf.obs[step].flatten(0, 1), h[:, 0]], -1))   # slot the env wrote: device tensors, no host hop
                logits, value, rnn = out[:, :cfg.n_actions], out[:, cfg.n_actions:cfg.n_actions + 1], torch.tanh(out[:, None, cfg.n_actions + 1:])
                dist = torch.distributions.Categorical(logits=logits)
                action = dist.sample()[:, None]                                  # int64 [N*A, 1], as policy.get_actions returns it (:346-355)
                buf.insert_step(action.view(N, A).to(torch.int32), values=value, actions=action, action_log_probs=dist.log_prob(action[:, 0])[:, None],
                                rnn_states=rnn, rnn_states_critic=rnn)          # envs.step + buffer.insert (:82-83, :384-428), learner fields in one launch
            buf.compute_returns(head(torch.cat([buf.obs[T].flatten(0, 1), buf.rnn_states[T].flatten(0, 1)[:, 0]], -1))[:, cfg.n_actions].view(N, A, 1))
            advantages = buf.normalized_advantages()
            for sample in buf.recurrent_generator(advantages, 2, min(T, 4)):     # the reference's 16-tuple; learner slots from the buffer
                n_mb += sample[6] is not None and sample[13] is not None
            buf.after_update()
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    return dict(path="device-resident, policy in the loop", env_steps_per_s=N * episodes * T / dt, mean_step_reward=float(buf.rewards.mean()),
                minibatches_with_learner_fields=n_mb,
                shapes=dict(obs=tuple(buf.obs.shape), node_obs=tuple(buf.node_obs.shape), adj=tuple(buf.adj.shape), rnn_states=tuple(buf.rnn_states.shape)))


def device_act_loop(args, episodes, hidden_size=16):
    """Shape (3) with the head inside the loop (`act_step`): the stand-in policy hands over its LOGITS; one launch masks them with the
    availability of the step (from dones[step - 1]), draws one action per (env, agent) and writes actions[step] / action_log_probs[step] in place; then the
    env step, the masks and one launch for values and RNN states. After the rollout, the first minibatch of the unchanged policy is put through
    `gmpe.ppo_losses`: its importance weights are exactly 1."""
    import torch
    from gmpe.engine import GmpeEngine
    from gmpe.rollout import DeviceRolloutBuffer
    from gmpe.config import config_from_args
    cfg = config_from_args(args)
    eng = GmpeEngine(cfg, adj_compact=True)
    run_args = argparse.Namespace(gamma=0.99, gae_lambda=0.95, use_gae=True, use_proper_time_limits=False, use_valuenorm=False, use_popart=False,
                                  recurrent_N=1, hidden_size=hidden_size)
    buf = DeviceRolloutBuffer(eng, args.episode_length, policy_fields="all", learner_fields="all", args=run_args)
    buf.warmup()
    T, N, A, K = args.episode_length, cfg.num_envs, cfg.num_agents, cfg.n_actions
    torch.manual_seed(0)
    head = torch.nn.Linear(cfg.obs_dim + hidden_size, K + 1 + hidden_size).to(eng.device)
    ratio_is_one = True
    torch.cuda.synchronize(); t0 = time.perf_counter()
    with torch.no_grad():
        for ep in range(episodes):
            kept = []
            for step in range(T):
                h = buf.rnn_states[step].flatten(0, 1)
                out = head(torch.cat([buf.obs[step].flatten(0, 1), h[:, 0]], -1))
                logits, value, rnn = out[:, :K].contiguous(), out[:, K:K + 1], torch.tanh(out[:, None, K + 1:])
                buf.act_step(logits, value, rnn_states=rnn, rnn_states_critic=rnn)   # head + envs.step + buffer.insert: no Categorical, no .to(int32)
                kept.append(logits)
            buf.compute_returns(head(torch.cat([buf.obs[T].flatten(0, 1), buf.rnn_states[T].flatten(0, 1)[:, 0]], -1))[:, K].view(N, A, 1))
            advantages = buf.normalized_advantages()
            f = dict(actions=buf.actions[0].view(N * A, 1), value_preds=buf.value_preds[0].view(N * A, 1), returns=buf.returns[0].view(N * A, 1),
                     active_masks=buf.active_masks[0].view(N * A, 1), old_action_log_probs=buf.action_log_probs[0].view(N * A, 1),
                     adv_targ=advantages[0].view(N * A, 1), available_actions=buf.available_actions[1].view(N * A, K))
            res = gmpe.ppo_losses(kept[0], buf.value_preds[0].view(N * A, 1), f, run_args)
            ratio_is_one = ratio_is_one and bool((res.imp_weights == 1.0).all())
            buf.after_update()
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    return dict(path="device-resident, action head in the loop", env_steps_per_s=N * episodes * T / dt, mean_step_reward=float(buf.rewards.mean()),
                act_draw=buf.act_draw, ratio_exactly_one=ratio_is_one,
                shapes=dict(obs=tuple(buf.obs.shape), actions=tuple(buf.actions.shape), action_log_probs=tuple(buf.action_log_probs.shape)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--agents", type=int, default=10)
    ap.add_argument("--episode-length", type=int, default=25)
    ap.add_argument("--episodes", type=int, default=3)
    ap.add_argument("--scenario", default="nav_metered_one_goal_graph_rotate_tube_july")
    a = ap.parse_args(argv)
    args = reference_args(a.envs, a.agents, a.episode_length, a.scenario)
    out = [drop_in_loop(args, a.episodes), device_loop(args, a.episodes), device_closed_loop(args, a.episodes)]
    for r in out + [device_act_loop(args, a.episodes)]:
        print(r)
    return out                                                                   # the three env-side shapes; shape (4) is printed, and callable on its own


if __name__ == "__main__":
    main()
