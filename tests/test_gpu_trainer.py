"""gmpe.policy.ppo_update, train, actor_forward and critic_forward against the REFERENCE'S OWN trainer: the float64 run of GR_MAPPO.ppo_update /
GR_MAPPO.train on GR_Actor / GR_Critic that tests/golden/make_trainer_fixture.py recorded (its one swap: gnn_new, replaced by gnn_lib's restatement).
The networks are tests/trainer_lib.py's mirrors — the reference's attribute names, its state_dict loaded strictly, its never-trained fc_h included —,
which tests/test_trainer_host.py pins to that run at 1e-14 on the CPU. Where tests/test_gpu_ppo_update.py compares the composition with the same
device calls written out a second time, these tests would notice a wrong reading of graph_mappo.py between the layers: which masks reach the RNN,
which observation reaches the critic, where value_loss_coef goes, which set is clipped and which is stepped after a PopArt replace, how train_info is
averaged.

The rule (trainer_lib): err = max|a - t| / max|t| per network and kind on the concatenated tensors, and per scalar; err_dev <= 4 * err_ref + 2^-23,
err_ref <= 1e-5 from the reference's float32 run. Cases: three consecutive updates on three samples of 6 x 5 rows (E = 7, K = 25).

Measured (one run, one MI355X): every array and scalar holds; the worst err_dev / bound is 0.87 (no-clip, critic_grad_norm after the second
update: a float32 scalar, an ulp off a truth whose err_ref is 1e-8), the worst over the concatenated arrays 0.37 (train-recurrent, the actor's
exp_avg), over the forward record 0.26."""
import numpy as np
import pytest
import torch

import trainer_lib as TL
from gmpe import policy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy(), np.float32).reshape(-1).view(np.uint32)


def device_update(actor, critic, aopt, copt, s, args, vn, update_actor):
    u = policy.ppo_update(actor, critic, aopt, copt, s, args, vn, update_actor)
    assert isinstance(u, policy.PPOUpdate) and u._fields[:6] == TL.SCALARS
    return tuple(u[:6]), u.imp_weights


@pytest.mark.parametrize("case", list(TL.CASES))
def test_three_ppo_updates_end_where_the_references_trainer_ends(case):
    fx = TL.load(case)
    scalars, imps, got, (actor, critic, aopt, copt, vn) = TL.run_updates(fx, device_update, DEV, torch.float32)
    torch.cuda.synchronize()
    worst = TL.compare(fx, scalars, got, TL.SCALARS, case, TL.bound, imps)
    print("%s worst err_dev / bound %.3g" % (case, worst))
    # fc_h never runs: no gradient, no state, and the bits it was loaded with
    for tag, net, opt in (("actor", actor, aopt), ("critic", critic, copt)):
        init = fx["init"]["critic_popart" if tag == "critic" and case == "popart" else tag]
        for k, p in net.base.mlp.fc_h.named_parameters():
            assert p.grad is None and p not in opt.state and np.array_equal(bits(p), bits(torch.from_numpy(init["base.mlp.fc_h." + k]))), (tag, k)
    if case == "no-actor":
        assert len(aopt.state) == 0 and all(np.array_equal(bits(p), bits(torch.from_numpy(fx["init"]["actor"][k]))) for k, p in actor.named_parameters())
    if case == "popart":
        # the optimiser holds the v_out objects of the first call, stepped once; the critic's own are new, with neither gradient nor state
        held = [p for g in copt.param_groups for p in g["params"]]
        old = [p for p in held if all(p is not q for q in critic.parameters())]
        assert len(old) == 3 and sorted(float(copt.state[p]["step"]) for p in old if p in copt.state) == [1.0, 1.0]
        for p in (critic.v_out.weight, critic.v_out.bias, critic.v_out.stddev):
            assert p.grad is None and p not in copt.state and all(p is not q for q in held)


@pytest.mark.parametrize("case", list(TL.TRAIN_CASES))
def test_train_ends_where_the_references_train_ends(case):
    """policy.train over a buffer that replays what the reference's GraphReplayBuffer yielded to GR_MAPPO.train, and refuses any other generator
    call than the recorded one. The real DeviceRolloutBuffer generators are held to the reference's by tests/golden/minibatch_generators.npz
    (tests/test_gpu_minibatch.py); the feed-forward case's networks have no RNNLayer, as the reference builds them without use_recurrent_policy."""
    fx = TL.load(case)
    info, got = TL.run_train(fx, policy.train, DEV, torch.float32)
    torch.cuda.synchronize()
    worst = TL.compare(fx, info, got, TL.TRAIN_INFO, case, TL.bound)
    print("%s worst err_dev / bound %.3g" % (case, worst))


def test_the_forward_passes_give_the_references_actions_values_and_states():
    fx = TL.inputs()
    actor, critic, _, _, _ = TL.nets(fx, device=DEV)
    s = TL.sample_on(fx["samples"][0], DEV, torch.float32)
    actions, lp, h = policy.actor_forward(actor, s[1], s[2], s[3], s[4], s[6], s[11], s[15], True, seed=0, num_agents=TL.NB, draw=0)
    with torch.no_grad():
        values, hc = policy.critic_forward(critic, s[0], s[2], s[3], s[5], s[7], s[11])
    torch.cuda.synchronize()
    t = fx["forward"]
    assert actions.dtype == torch.int64 and np.array_equal(actions.cpu().numpy(), t["actions"])          # every row: no two logits within 1e-4
    rows = [(k, float(t["err_ref:" + k]), TL.err(v.double().cpu().numpy(), t[k])) for k, v in (("action_log_probs", lp), ("rnn_states", h), ("values", values),
                                                                                               ("rnn_states_critic", hc))]
    for k, e_ref, e_dev in rows:
        print("forward %-18s err_ref %.3g err_dev %.3g bound %.3g" % (k, e_ref, e_dev, TL.bound(e_ref)))
    print("forward worst err_dev / bound %.3g" % max(e_dev / TL.bound(e_ref) for _, e_ref, e_dev in rows))
    for k, e_ref, e_dev in rows:
        assert e_ref <= TL.CAP and e_dev <= TL.bound(e_ref), (k, e_dev, e_ref)
