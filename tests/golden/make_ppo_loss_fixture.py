"""Golden vectors for the PPO loss arithmetic (gmpe_ppo_loss), produced by RUNNING the reference on the CPU:

    python tests/golden/make_ppo_loss_fixture.py        # writes tests/golden/ppo_loss.npz

What runs (the reference's own code on the CPU; imports and stubs as in make_returns_fixture.py):
  * `GR_MAPPO.ppo_update` (onpolicy/algorithms/graph_mappo.py:121-278) of a real `GR_MAPPO(args, policy)` on a stub policy whose PARAMETERS are the
    logits [B, K] and the values [B, 1] (SGD with lr 0, max_grad_norm 1e30, so clip_grad_norm_ multiplies by exactly 1): after each update `.grad` holds
    the reference's gradient of (policy_loss - dist_entropy * entropy_coef) with respect to the logits and of value_loss with respect to the values
    (the critic's .grad is divided back by value_loss_coef = 1);
  * the stub's evaluate_actions calls the reference's `ACTLayer.evaluate_actions` (onpolicy/algorithms/utils/act.py:212-220) of an
    `ACTLayer(Discrete(K), K, ...)` whose `Categorical` (distributions.py:84-91) has its linear layer set to the identity, so x is the logits, and passes
    active_masks exactly when use_policy_active_masks is set, as GR_Actor.evaluate_actions does (graph_actor_critic.py:254-256);
  * the trainer's own `ValueNorm(1)` (onpolicy/utils/valuenorm.py), carried across three consecutive minibatches; its three tensors are stored after each.
Inputs are the seeded families of tests/ppo_loss_lib.py; the vectors are data only.
"""
import argparse
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_buffer_fixture as MB  # noqa: E402
import ppo_loss_lib as P  # noqa: E402

# name -> (K, family, cfg keywords): both settings of the four boolean flags, huber delta 10 and a small one, K in {5, 25}, with and without ValueNorm
CASES = {
    "a": (25, "generic", dict(valuenorm=True)),
    "b": (5, "generic", dict(pm=False, vm=False, clipped=False, huber=False, valuenorm=True)),
    "c": (25, "edges", dict(huber_delta=0.5)),
    "d": (5, "ties", dict(vm=False, huber=False)),
    "e": (5, "edges", dict(pm=False, clipped=False, huber_delta=0.5, valuenorm=True)),
}
ROWS, MINIBATCHES = 96, 3


def load_reference():
    MB.load_reference()
    MB._stub("onpolicy.algorithms.graph_MAPPOPolicy", GR_MAPPOPolicy=object)       # imports torch_geometric (absent here); ppo_update never touches the class
    from onpolicy.algorithms.graph_mappo import GR_MAPPO
    from onpolicy.algorithms.utils.act import ACTLayer
    return GR_MAPPO, ACTLayer


def run_case(GR_MAPPO, ACTLayer, K, fam, kw):
    import gym
    import torch
    c = P.cfg(**kw)
    args = argparse.Namespace(clip_param=c.clip_param, ppo_epoch=1, num_mini_batch=1, data_chunk_length=10, value_loss_coef=1.0,
                              entropy_coef=c.entropy_coef, max_grad_norm=1e30, huber_delta=c.huber_delta, use_recurrent_policy=False,
                              use_naive_recurrent_policy=False, use_max_grad_norm=True, use_clipped_value_loss=c.use_clipped_value_loss,
                              use_huber_loss=c.use_huber_loss, use_popart=False, use_valuenorm=c.use_valuenorm,
                              use_value_active_masks=c.use_value_active_masks, use_policy_active_masks=c.use_policy_active_masks)
    act = ACTLayer(gym.spaces.Discrete(K), K, True, 0.01)
    with torch.no_grad():
        act.action_out.linear.weight.copy_(torch.eye(K))
        act.action_out.linear.bias.zero_()
    seen = {}

    class Policy(object):
        def __init__(self):
            self.logits = torch.nn.Parameter(torch.zeros(ROWS, K))
            self.values = torch.nn.Parameter(torch.zeros(ROWS, 1))
            self.actor = types.SimpleNamespace(parameters=lambda: [self.logits])
            self.critic = types.SimpleNamespace(parameters=lambda: [self.values])
            self.actor_optimizer = torch.optim.SGD([self.logits], lr=0.0)
            self.critic_optimizer = torch.optim.SGD([self.values], lr=0.0)

        def evaluate_actions(self, share_obs, obs, node_obs, adj, agent_id, share_agent_id, rnn_states, rnn_states_critic, action, masks,
                             available_actions=None, active_masks=None):
            to = lambda a: None if a is None else torch.from_numpy(a)
            logp, ent = act.evaluate_actions(self.logits, to(action), to(available_actions),
                                             active_masks=active_masks if c.use_policy_active_masks else None)
            seen["action_log_probs"] = logp.detach().numpy().copy()
            return self.values, logp, ent
    policy = Policy()
    trainer = GR_MAPPO(args, policy)
    trainer.update_counter = 0
    rec = dict(K=K, family=fam, cfg=np.array([c.clip_param, c.huber_delta, c.entropy_coef], np.float64),
               flags=np.array([c.use_policy_active_masks, c.use_value_active_masks, c.use_clipped_value_loss, c.use_huber_loss, c.use_valuenorm]))
    state = P.fresh_state() if c.use_valuenorm else None
    for i in range(MINIBATCHES):
        inp = P.family(fam, ROWS, K, seed=100 + i, c=c, state=state, masks="mixed")
        with torch.no_grad():
            policy.logits.copy_(torch.from_numpy(inp["logits"]))
            policy.values.copy_(torch.from_numpy(inp["values"]))
        sample = (None,) * 8 + (inp["actions"], inp["value_preds"], inp["returns"], None, inp["active_masks"], inp["old_action_log_probs"],
                                inp["adv_targ"], inp["available_actions"])
        value_loss, _, policy_loss, dist_entropy, _, imp_weights, _, _ = trainer.ppo_update(sample)
        out = dict(value_loss=value_loss, policy_loss=policy_loss, dist_entropy=dist_entropy, imp_weights=imp_weights,
                   ratio_mean=imp_weights.mean(), grad_logits=policy.logits.grad, grad_values=policy.values.grad / args.value_loss_coef)
        for k, v in inp.items():
            rec["%d_in_%s" % (i, k)] = v
        for k, v in out.items():
            rec["%d_%s" % (i, k)] = v.detach().numpy().copy()
        rec["%d_action_log_probs" % i] = seen["action_log_probs"]
        if c.use_valuenorm:
            vn = trainer.value_normalizer
            state = dict(running_mean=vn.running_mean.detach().numpy().copy(), running_mean_sq=vn.running_mean_sq.detach().numpy().copy(),
                         debiasing_term=vn.debiasing_term.detach().numpy().copy())
            for k, v in state.items():
                rec["%d_state_%s" % (i, k)] = v
    return rec


def main():
    GR_MAPPO, ACTLayer = load_reference()
    d = {}
    for name, (K, fam, kw) in CASES.items():
        for k, v in run_case(GR_MAPPO, ACTLayer, K, fam, kw).items():
            d["%s_%s" % (name, k)] = v
    p = os.path.join(HERE, "ppo_loss.npz")
    np.savez_compressed(p, **d)
    print(p, os.path.getsize(p), len(d))


if __name__ == "__main__":
    main()
