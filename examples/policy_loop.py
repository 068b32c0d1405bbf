"""The reference runner's whole iteration (onpolicy/runner/shared/graph_mpe_runner.py:57-129) with the policy in the loop, on the device:

    for episode in range(episodes):
        for step in range(episode_length):
            collect / collect_with_mask, envs.step, insert      ->  gmpe.policy.collect_step(actor, critic, buffer)
        compute()                                               ->  gmpe.policy.compute(critic, buffer, value_normalizer)
        train()                                                 ->  gmpe.policy.train(actor, critic, actor_optimizer, critic_optimizer, buffer, args, ...)
        buffer.after_update()

written out once (`by_pieces`) and as the one call that does the same (`gmpe.policy.iteration`). The networks are the caller's GR_Actor / GR_Critic,
read by their attribute names; here they are stand-ins with those names (tests/test_gpu_policy.py's mirror modules with the shipped GNN and head
weights), because the reference's modules need torch_geometric. Nothing between warmup() and the printed scalars is copied to the host.

    python examples/policy_loop.py --envs 64 --agents 3 --episodes 3 [--popart] [--captured] [--run]

With --captured both halves of every iteration are replayed graphs: the rollout is gmpe.policy.CapturedRollout.replay — the episode's collect_steps and
compute captured once, one launch per episode — and train() is gmpe.policy.CapturedUpdate.train: one ppo_update captured as a graph, replayed per
minibatch. With --run --captured the same is gmpe.policy.run(..., captured=True).
With --run the same training is the reference's whole run() loop as one call, gmpe.policy.run, with three printing callbacks: the linear lr decay, the
iterations, the `agent{i}/...` means of process_infos + log_env at the log interval (gmpe.env_infos), the deterministic eval episode on a second
engine at the eval interval (gmpe.policy.eval_episode) and the saves. Only the callbacks read values back.
"""
import argparse
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))        # the stand-in networks
import gmpe  # noqa: E402


def runner_args(popart, episode_length):
    """what the buffer, the losses and train read of the runner's args, with the reference's defaults"""
    return types.SimpleNamespace(
        gamma=0.99, gae_lambda=0.95, use_gae=True, use_proper_time_limits=False, use_popart=popart, use_valuenorm=not popart, clip_param=0.2,
        huber_delta=10.0, entropy_coef=0.01, use_policy_active_masks=True, use_value_active_masks=True, use_clipped_value_loss=True, use_huber_loss=True,
        use_max_grad_norm=True, max_grad_norm=10.0, value_loss_coef=1.0, use_recurrent_policy=True, use_naive_recurrent_policy=False, ppo_epoch=2,
        num_mini_batch=1, data_chunk_length=10 if episode_length % 10 == 0 else episode_length, recurrent_N=1, hidden_size=64)


def networks(cfg, eng, popart, dev):
    import torch
    import gnn_lib as G
    import head_lib as HL
    import trainer_lib as TL
    from test_gpu_policy import _Net
    key = G.ACTOR if int(cfg.node_feats) == 7 else G.ROTATE
    actor = _Net(key, eng.D, "act").to(dev)
    critic = _Net(key, eng.D, "popart" if popart else "v_out", seed=12).to(dev)
    if popart:
        class PopArt(HL.PopArt):                        # the reference's PopArt has debiased_mean_var (popart.py:85-89); the stand-in needs it too
            def debiased_mean_var(self):
                mean = self.mean / self.debiasing_term.clamp(min=self.epsilon)
                return mean, (self.mean_sq / self.debiasing_term.clamp(min=self.epsilon) - mean ** 2).clamp(min=1e-2)
        normalizer = critic.v_out = PopArt(dev)         # graph_mappo.py:63-64: the value normaliser IS the critic's output layer
        params = list(critic.parameters()) + [critic.v_out.weight, critic.v_out.bias]
    else:
        class ValueNorm(TL.ValueNorm):
            def running_mean_var(self):                 # valuenorm.py:48-55
                mean = self.running_mean / self.debiasing_term.clamp(min=self.epsilon)
                return mean, (self.running_mean_sq / self.debiasing_term.clamp(min=self.epsilon) - mean ** 2).clamp(min=1e-2)
        normalizer, params = ValueNorm(dev), list(critic.parameters())
    adam = lambda ps: torch.optim.Adam(ps, lr=7e-4, eps=1e-5, weight_decay=0)
    return actor, critic, adam(list(actor.parameters())), adam(params), normalizer


def by_pieces(actor, critic, aopt, copt, buf, args, normalizer):
    """one iteration, call by call"""
    from gmpe import policy
    for _ in range(buf.T):
        policy.collect_step(actor, critic, buf)         # get_actions on slot buf.step, the env step, the masks, the learner fields
    policy.compute(critic, buf, normalizer)             # get_values on the last slot, then compute_returns
    info = policy.train(actor, critic, aopt, copt, buf, args, normalizer, value_head="device")
    info["average_episode_rewards"] = buf.rewards.mean() * buf.T
    buf.after_update()
    return info


def captured(caps, actor, critic, aopt, copt, buf, args, normalizer):
    """one iteration of two replayed graphs: the rollout (gmpe.policy.CapturedRollout, built at the first call on the warmed-up buffer: the graph is
    fixed to the buffer's arrays and the networks' parameters, whose values it follows) and the updates (gmpe.policy.CapturedUpdate, built at the
    first call from a minibatch of the first rollout: the graph is fixed to that minibatch's shapes) -> (info, (the CapturedRollout, the CapturedUpdate))"""
    from gmpe import policy
    roll, cap = caps or (None, None)
    if roll is None:
        roll = policy.CapturedRollout(actor, critic, buf, normalizer)
    roll.replay()
    if cap is None:
        sample = next(iter(buf.recurrent_generator(buf.normalized_advantages(normalizer), args.num_mini_batch, args.data_chunk_length)))
        cap = policy.CapturedUpdate(actor, critic, aopt, copt, sample, args, normalizer, value_head="device")
    info = cap.train(buf)
    info["average_episode_rewards"] = buf.rewards.mean() * buf.T
    buf.after_update()
    return info, (roll, cap)


def run_whole(o, actor, critic, aopt, copt, buf, args, normalizer, cfg):
    """GMPERunner.run as gmpe.policy.run plus the callbacks a training script still writes"""
    from gmpe import policy
    from gmpe.engine import GmpeEngine
    args.episode_length, args.n_rollout_threads = o.episode_length, o.envs
    args.save_interval, args.log_interval, args.eval_interval, args.use_eval = 2, 1, 2, True
    args.use_linear_lr_decay, args.lr, args.critic_lr = True, 7e-4, 7e-4
    eval_engine = GmpeEngine(gmpe.make_config(num_envs=o.envs, num_agents=o.agents, episode_length=o.episode_length, seed=2), device=0)

    def on_log(total_num_steps, train_infos, env_infos):
        print("steps %d train: %s" % (total_num_steps, {k: round(float(v), 5) for k, v in train_infos.items()}))
        for a in range(o.agents):
            keys = ["agent%d/%s" % (a, k) for k in ("individual_rewards", "dist_to_goal", "time_to_goal", "num_agent_collisions")]
            print("steps %d %s" % (total_num_steps, "  ".join("%s %.4f" % (k, float(env_infos[k])) for k in keys)))

    def on_eval(total_num_steps, eval_infos):
        print("steps %d eval average episode rewards of agent: %.5f" % (total_num_steps, float(eval_infos["mean"])))

    def on_save(episode):
        print("episode %d: save (lr %.3g)" % (episode, aopt.param_groups[0]["lr"]))

    policy.run(actor, critic, aopt, copt, buf, args, normalizer, episodes=o.episodes, eval_engine=eval_engine, on_log=on_log, on_eval=on_eval,
               on_save=on_save, value_head="device", captured=o.captured)
    eval_engine.check_errors()
    eval_engine.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--agents", type=int, default=3)
    ap.add_argument("--episode-length", type=int, default=20)
    ap.add_argument("--episodes", type=int, default=3)
    ap.add_argument("--popart", action="store_true", help="--use_popart: the critic's v_out is the value normaliser")
    ap.add_argument("--captured", action="store_true", help="every rollout and every update is a replay of a captured graph (gmpe.policy.CapturedRollout.replay, "
                    "gmpe.policy.CapturedUpdate.train; with --popart the rescaled layer is written in place, install=\"in_place\")")
    ap.add_argument("--run", action="store_true", help="the whole loop as one call: gmpe.policy.run with printing callbacks")
    o = ap.parse_args()
    import torch
    from gmpe import policy
    from gmpe.engine import GmpeEngine
    from gmpe.rollout import DeviceRolloutBuffer
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: the kernels have no CPU fallback")
    dev = "cuda:0"
    cfg = gmpe.make_config(num_envs=o.envs, num_agents=o.agents, episode_length=o.episode_length, seed=1)
    eng = GmpeEngine(cfg, device=0)
    args = runner_args(o.popart, o.episode_length)
    actor, critic, aopt, copt, normalizer = networks(cfg, eng, o.popart, dev)
    buf = DeviceRolloutBuffer(eng, o.episode_length, use_centralized_V=False, policy_fields="all", learner_fields="all", args=args)
    if o.run:
        run_whole(o, actor, critic, aopt, copt, buf, args, normalizer, cfg)
        eng.check_errors()
        eng.close()
        return
    buf.warmup()
    cap = None
    for ep in range(o.episodes):
        t0 = time.perf_counter()
        if o.captured:
            (info, cap), how = captured(cap, actor, critic, aopt, copt, buf, args, normalizer), "captured rollout and updates"
        elif ep % 2 == 0:
            info, how = by_pieces(actor, critic, aopt, copt, buf, args, normalizer), "by pieces"
        else:
            info, how = policy.iteration(actor, critic, aopt, copt, buf, args, normalizer, value_head="device"), "policy.iteration"
        line = {k: round(float(v), 5) for k, v in info.items()}             # the one read-back of the iteration
        print("episode %d (%s) %.0f ms: %s" % (ep, how, (time.perf_counter() - t0) * 1e3, line))
    eng.check_errors()
    eng.close()


if __name__ == "__main__":
    main()
