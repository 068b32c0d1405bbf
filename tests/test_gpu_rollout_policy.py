"""gmpe.policy.get_actions and compute, with DeviceRolloutBuffer.insert_external's learner fields between them, against the REFERENCE'S OWN runner: the
float64 run of GMPERunner.collect / collect_with_mask / insert / compute on GR_Actor / GR_Critic that tests/golden/make_rollout_fixture.py recorded
(its one swap: gnn_new, replaced by gnn_lib's restatement; deterministic=True, the reference's mode()). The env outputs are the fixture's prescribed
ones, replayed through a real DeviceRolloutBuffer of the same config, so what is held to the reference is everything between them over T = 6 steps:
which slot each chain reads, the carried RNN states and their zeroed done rows (an agent done alone at step 2, a whole env at step 3), the masks that
reach the RNN, the stop-action rows of collect_with_mask, the value normaliser inside compute_returns.

Exact: actions, available_actions, masks, active_masks. The rule for the rest (tests/trainer_lib.py's): err(a, t) = max|a - t| / max|t| per array,
err_dev <= 4 * err_ref + 2^-23, err_ref <= 1e-5 from the reference's float32 run."""
import types

import numpy as np
import pytest
import torch

import rollout_lib as RL
from gmpe import policy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, A, T = RL.N, RL.A, RL.T
ROWS = N * A


@pytest.mark.parametrize("case", RL.CASES)
def test_the_rollout_ends_where_the_references_runner_ends(case):
    from gmpe.engine import GmpeEngine
    from gmpe.rollout import DeviceRolloutBuffer
    fx = RL.load(case)
    env, truth = fx["env"], fx["truth"]
    cfg = RL.config()
    eng = GmpeEngine(cfg, device=0, adj_compact=False)
    assert tuple(env["obs"].shape) == (T + 1, N, A, eng.D) and tuple(env["adj"].shape) == (T + 1, N, A, eng.E, eng.E)
    actor, critic, vn = RL.nets(fx, case, DEV)
    buf = DeviceRolloutBuffer(eng, T, use_centralized_V=False, policy_fields="all", learner_fields="all", args=types.SimpleNamespace(**fx["args"]),
                              recurrent_N=1, hidden_size=64)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    # the reset's outputs go to slot 0, as warmup() puts them there
    buf.obs[0].copy_(dev(env["obs"][0])), buf._node_obs[0].copy_(dev(env["node_obs"][0])), buf._adj[0].copy_(dev(env["adj"][0]))
    buf.agent_id[0].copy_(dev(env["agent_id"][0]).to(torch.int32))
    got = {k: [] for k in ("values", "actions", "action_log_probs")}
    for t in range(T):
        assert buf.step == t
        s = policy._slot_rows(buf, t)
        buf.available_actions_for(t)
        values, actions, logp, h, hc = policy.get_actions(actor, critic, s["share_obs"], s["obs"], s["node_obs"], s["adj"], s["agent_id"], s["share_agent_id"],
                                                          s["rnn_states"], s["rnn_states_critic"], s["masks"], None, True,
                                                          dones_prev=buf.dones[t - 1].view(ROWS) if t else None, seed=cfg.seed, env_id_base=cfg.env_id_base,
                                                          num_agents=A, draw=t)
        buf.insert_external(dev(env["obs"][t + 1]), dev(env["agent_id"][t + 1]), dev(env["node_obs"][t + 1]), dev(env["adj"][t + 1]),
                            dev(env["rewards"][t]), dev(env["dones"][t]), values, actions=actions, action_log_probs=logp, rnn_states=h,
                            rnn_states_critic=hc)
        for k, v in zip(("values", "actions", "action_log_probs"), (values, actions, logp)):
            got[k].append(v.view(N, A, 1))
    policy.compute(critic, buf, vn)
    torch.cuda.synchronize()
    got = {k: torch.stack(v).cpu().numpy() for k, v in got.items()}
    for k in ("rnn_states", "rnn_states_critic", "value_preds", "returns", "masks", "active_masks", "available_actions"):
        got[k] = getattr(buf, k).cpu().numpy()
    assert np.array_equal(buf.actions.cpu().numpy(), got["actions"].astype(np.float32))             # what was stored is what was returned
    for k in RL.EXACT:
        assert got[k].shape == truth[k].shape and np.array_equal(got[k].astype(np.float64), truth[k].astype(np.float64)), k
    dn = env["dones"]
    assert (got["rnn_states"][1:][dn] == 0).all() and (got["rnn_states_critic"][1:][dn] == 0).all()     # the zeroed rows are zero, not small
    rows = [(k, fx["err_ref"][k], RL.err(got[k].astype(np.float64), truth[k])) for k in RL.CLOSE]
    for k, e_ref, e_dev in rows:
        print("%s %-18s err_ref %.3g err_dev %.3g bound %.3g" % (case, k, e_ref, e_dev, RL.bound(e_ref)))
    print("%s worst err_dev / bound %.3g" % (case, max(e_dev / RL.bound(e_ref) for _, e_ref, e_dev in rows)))
    for k, e_ref, e_dev in rows:
        assert got[k].shape == truth[k].shape and e_ref <= RL.CAP and e_dev <= RL.bound(e_ref), (k, e_dev, e_ref)
    eng.check_errors()
    eng.close()
