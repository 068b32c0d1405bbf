"""Golden vectors for the PPO loss arithmetic with PopArt (gmpe_ppo_loss_popart), produced by RUNNING the reference on the CPU:

    python tests/golden/make_popart_fixture.py        # writes tests/golden/popart_loss.npz

What runs (the reference's own code; imports and stubs as in make_ppo_loss_fixture.py):
  * `GR_MAPPO.ppo_update` of a real `GR_MAPPO(args, policy)` with use_popart=True on a stub policy whose PARAMETERS are the logits [ROWS, K] and the
    critic FEATURES [ROWS, H]; the stub's critic has `v_out = PopArt(H, 1)` (onpolicy/algorithms/utils/popart.py), so trainer.value_normalizer is that
    layer (graph_mappo.py:63-64) and evaluate_actions returns v_out(features), formed before cal_value_loss updates the layer;
  * SGD with lr 0 over features, weight and bias, max_grad_norm 1e30 (clip_grad_norm_ multiplies by exactly 1);
  * three consecutive minibatches per case. PopArt.update replaces weight and bias by new Parameters, so the gradients of a minibatch land on the objects
    that were there before it: references to them are kept and their .grad stored.
Inputs are the seeded families of tests/popart_lib.py; the vectors are data only.
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
import make_ppo_loss_fixture as MP  # noqa: E402
import popart_lib as PL  # noqa: E402

# name -> (ROWS, K, H, exact, cfg keywords)
CASES = {
    "g8": (96, 25, 8, False, dict()),
    "g64": (96, 5, 64, False, dict(pm=False, vm=False, clipped=False, huber=False)),
    "exact": (128, 5, 64, True, dict()),
}
MINIBATCHES = 3


def run_case(GR_MAPPO, ACTLayer, PopArt, ROWS, K, H, exact, kw):
    import gym
    import torch
    c = PL.cfg(**kw)
    args = argparse.Namespace(clip_param=c.clip_param, ppo_epoch=1, num_mini_batch=1, data_chunk_length=10, value_loss_coef=1.0,
                              entropy_coef=c.entropy_coef, max_grad_norm=1e30, huber_delta=c.huber_delta, use_recurrent_policy=False,
                              use_naive_recurrent_policy=False, use_max_grad_norm=True, use_clipped_value_loss=c.use_clipped_value_loss,
                              use_huber_loss=c.use_huber_loss, use_popart=True, use_valuenorm=False,
                              use_value_active_masks=c.use_value_active_masks, use_policy_active_masks=c.use_policy_active_masks)
    act = ACTLayer(gym.spaces.Discrete(K), K, True, 0.01)
    with torch.no_grad():
        act.action_out.linear.weight.copy_(torch.eye(K))
        act.action_out.linear.bias.zero_()
    seen = {}
    init = PL.fresh_popart(H, seed=ROWS + K, exact=exact)

    class Policy(object):
        def __init__(self):
            self.logits = torch.nn.Parameter(torch.zeros(ROWS, K))
            self.features = torch.nn.Parameter(torch.zeros(ROWS, H))
            v_out = PopArt(H, 1)
            with torch.no_grad():
                v_out.weight.copy_(torch.from_numpy(init["weight"]))
                v_out.bias.copy_(torch.from_numpy(init["bias"]))
            self.refs = [v_out.weight, v_out.bias]                          # the objects the next minibatch's gradients land on
            self.actor = types.SimpleNamespace(parameters=lambda: [self.logits])
            self.critic = types.SimpleNamespace(v_out=v_out, parameters=lambda: [self.features] + self.refs)
            self.actor_optimizer = torch.optim.SGD([self.logits], lr=0.0)
            self.critic_optimizer = torch.optim.SGD([self.features, v_out.weight, v_out.bias], lr=0.0)

        def evaluate_actions(self, share_obs, obs, node_obs, adj, agent_id, share_agent_id, rnn_states, rnn_states_critic, action, masks,
                             available_actions=None, active_masks=None):
            to = lambda a: None if a is None else torch.from_numpy(a)
            logp, ent = act.evaluate_actions(self.logits, to(action), to(available_actions),
                                             active_masks=active_masks if c.use_policy_active_masks else None)
            values = self.critic.v_out(self.features)                       # graph_actor_critic.py:395
            seen["action_log_probs"] = logp.detach().numpy().copy()
            seen["values"] = values.detach().numpy().copy()
            return values, logp, ent
    policy = Policy()
    trainer = GR_MAPPO(args, policy)
    trainer.update_counter = 0
    v_out = policy.critic.v_out
    assert trainer.value_normalizer is v_out
    rec = dict(K=K, H=H, cfg=np.array([c.clip_param, c.huber_delta, c.entropy_coef], np.float64),
               flags=np.array([c.use_policy_active_masks, c.use_value_active_masks, c.use_clipped_value_loss, c.use_huber_loss]))
    for k, v in init.items():
        rec["init_%s" % k] = v
    state = init
    for i in range(MINIBATCHES):
        inp = PL.exact_inputs(ROWS, K, H, c, seed=100 + i) if exact else PL.family(ROWS, K, H, state, c, seed=100 + i)
        inp.pop("values")
        with torch.no_grad():
            policy.logits.copy_(torch.from_numpy(inp["logits"]))
            policy.features.copy_(torch.from_numpy(inp["features"]))
        policy.refs = [v_out.weight, v_out.bias]
        for p in policy.refs:
            p.grad = None
        sample = (None,) * 8 + (inp["actions"], inp["value_preds"], inp["returns"], None, inp["active_masks"], inp["old_action_log_probs"],
                                inp["adv_targ"], inp["available_actions"])
        value_loss, _, policy_loss, dist_entropy, _, imp_weights, _, _ = trainer.ppo_update(sample)
        assert v_out.weight is not policy.refs[0] and v_out.bias is not policy.refs[1]
        out = dict(value_loss=value_loss, policy_loss=policy_loss, dist_entropy=dist_entropy, imp_weights=imp_weights, ratio_mean=imp_weights.mean(),
                   grad_logits=policy.logits.grad, grad_features=policy.features.grad / args.value_loss_coef,
                   grad_weight=policy.refs[0].grad / args.value_loss_coef, grad_bias=policy.refs[1].grad / args.value_loss_coef)
        for k, v in inp.items():
            rec["%d_in_%s" % (i, k)] = v
        for k, v in out.items():
            rec["%d_%s" % (i, k)] = v.detach().numpy().copy()
        rec["%d_action_log_probs" % i] = seen["action_log_probs"]
        rec["%d_values" % i] = seen["values"]
        state = {k: getattr(v_out, k).detach().numpy().copy() for k in PL.STATE}
        assert float(state["mean_sq"].reshape(-1)[0]) - float(state["mean"].reshape(-1)[0]) ** 2 > 0        # the sqrt of step 4 stays real
        for k, v in state.items():
            rec["%d_state_%s" % (i, k)] = v
    return rec


def main():
    GR_MAPPO, ACTLayer = MP.load_reference()
    from onpolicy.algorithms.utils.popart import PopArt
    d = {}
    for name, (ROWS, K, H, exact, kw) in CASES.items():
        for k, v in run_case(GR_MAPPO, ACTLayer, PopArt, ROWS, K, H, exact, kw).items():
            d["%s_%s" % (name, k)] = v
    p = os.path.join(HERE, "popart_loss.npz")
    np.savez_compressed(p, **d)
    print(p, os.path.getsize(p), len(d))


if __name__ == "__main__":
    main()
