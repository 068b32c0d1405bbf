"""The rollout half of gmpe.policy — get_actions, get_values, collect_step, compute, rollout, iteration — against the same thing written by hand from the
public pieces: gnn_base, mlp_base, rnn_layer, action_logits, value_head, DeviceRolloutBuffer.act_step(logits, values, rnn_states=..., rnn_states_critic=...),
then get_values by hand and compute_returns. The composition adds no arithmetic, so every stored array of the two buffers must agree bit for bit over two
episodes joined by after_update, with dones inside the rollout (T = 9 steps of envs whose time limit is 6, as tests/test_gpu_act_buffer.py).
The networks are tests/test_gpu_policy.py's mirror modules, sized from the engine's config.
train(..., value_head="device") is held to the reference's own GR_MAPPO.train by tests/trainer_lib.py's rule, as tests/test_gpu_trainer.py holds the
default path: err_dev <= 4 * err_ref + 2^-23 on the critic's (and the actor's) clipped gradients, Adam state, parameters and on train_info."""
import types

import numpy as np
import pytest
import torch

import gmpe
import gnn_lib as G
import head_lib as HL
import trainer_lib as TL
from gmpe import policy
from test_gpu_act_buffer import ARRAYS, A, N, T, _same
from test_gpu_policy import DEV, K, _Net

pytestmark = pytest.mark.gpu
STORED = ARRAYS + ("returns", "advantages")
ROWS = N * A


class _ValueNorm(TL.ValueNorm):
    def running_mean_var(self):                             # valuenorm.py:48-55
        mean = self.running_mean / self.debiasing_term.clamp(min=self.epsilon)
        var = (self.running_mean_sq / self.debiasing_term.clamp(min=self.epsilon) - mean ** 2).clamp(min=1e-2)
        return mean, var


class _PopArt(HL.PopArt):
    def debiased_mean_var(self):                            # popart.py:85-89
        mean = self.mean / self.debiasing_term.clamp(min=self.epsilon)
        var = (self.mean_sq / self.debiasing_term.clamp(min=self.epsilon) - mean ** 2).clamp(min=1e-2)
        return mean, var


CASES = {"recurrent-valuenorm-cent": dict(rnn=True, norm="valuenorm", cent=True), "recurrent-popart-own": dict(rnn=True, norm="popart", cent=False),
         "no-rnn-plain-cent": dict(rnn=False, norm=None, cent=True)}


def _setup(rnn=True, norm=None, cent=True, buffers=2, **more_args):
    """`buffers` engines of one config (the same envs) with a warmed-up buffer each, one actor and one critic, the value normaliser"""
    from gmpe.engine import GmpeEngine
    from gmpe.rollout import DeviceRolloutBuffer
    cfg = gmpe.make_config(num_envs=N, num_agents=A, episode_length=6, seed=11)     # the time limit lies inside the rollout: dones occur
    engines = [GmpeEngine(cfg, device=0) for _ in range(buffers)]
    F = int(cfg.node_feats)
    key = G.ACTOR if F == 7 else G.ROTATE
    assert G.CONFIGS[key]["F"] == F and int(cfg.n_actions) == K
    actor = _Net(key, engines[0].D, "act").to(DEV)
    critic = _Net(key, engines[0].D if cent else 0, "popart" if norm == "popart" else "v_out", use_cent_obs=cent, seed=12).to(DEV)
    if not rnn:
        del actor.rnn, critic.rnn
    vn = None
    if norm == "popart":
        vn = critic.v_out = _PopArt(DEV)
        vn.mean.fill_(0.3), vn.mean_sq.fill_(0.7), vn.debiasing_term.fill_(0.5)
    elif norm == "valuenorm":
        vn = _ValueNorm(DEV)
        vn.running_mean.fill_(0.3), vn.running_mean_sq.fill_(0.7), vn.debiasing_term.fill_(0.5)
    args = types.SimpleNamespace(gamma=0.99, gae_lambda=0.95, use_gae=True, use_proper_time_limits=False, use_valuenorm=norm == "valuenorm",
                                 use_popart=norm == "popart", **more_args)
    bufs = [DeviceRolloutBuffer(e, T, use_centralized_V=False, policy_fields="all", learner_fields="all", args=args, recurrent_N=1, hidden_size=64)
            for e in engines]
    for b in bufs:
        b.warmup()
    return cfg, engines, bufs, actor, critic, vn


def _chains(actor, critic, B, t, cent, rnn):
    """the two chains on slot t of B, layer call by layer call -> (actor features, critic features, h, hc)"""
    E = int(B._node_obs.shape[-2])
    x, adj = B._node_obs[t].reshape(ROWS, E, -1), B._adj[t].reshape(-1, E, E)
    ids, masks = B.agent_id[t].reshape(ROWS), B.masks[t].reshape(ROWS, 1)
    obs, share_obs, share_ids = B.obs[t].reshape(ROWS, -1), B.share_obs[t].reshape(ROWS, -1), B.share_agent_id[t].reshape(ROWS)
    h = hc = None
    f = gmpe.mlp_base((obs, gmpe.gnn_base(x, adj, ids, actor.gnn_base)), actor.base)
    nbd_c = gmpe.gnn_base(x, adj, share_ids, critic.gnn_base)
    fc = gmpe.mlp_base((share_obs, nbd_c) if cent else nbd_c, critic.base)
    if rnn:
        f, h = gmpe.rnn_layer(f, B.rnn_states[t].reshape(ROWS, 1, 64), masks, actor.rnn)
        fc, hc = gmpe.rnn_layer(fc, B.rnn_states_critic[t].reshape(ROWS, 1, 64), masks, critic.rnn)
    return f, fc, h, hc


def _by_hand(actor, critic, B, vn, cent, rnn):
    """one episode: T steps of the layer calls and act_step, then get_values by hand and compute_returns"""
    with torch.no_grad():
        for t in range(T):
            assert B.step == t
            f, fc, h, hc = _chains(actor, critic, B, t, cent, rnn)
            B.act_step(gmpe.action_logits(f, actor.act), gmpe.value_head(fc, critic.v_out), rnn_states=h, rnn_states_critic=hc)
        _, fc, _, _ = _chains(actor, critic, B, T, cent, rnn)
        B.compute_returns(gmpe.value_head(fc, critic.v_out).view(N, A, 1), vn)


def _compare(ba, bb, what):
    torch.cuda.synchronize()
    dn = ba.dones.bool().cpu().numpy()
    assert dn.any() and not dn.all(), "%s: dones %d" % (what, dn.sum())
    for k in STORED:
        x, y = getattr(ba, k), getattr(bb, k)
        assert x is not None and y is not None, k
        _same(x, y, "%s %s" % (what, k))
    assert ba.step == bb.step == 0 and ba.act_draw == bb.act_draw


@pytest.mark.parametrize("case", list(CASES))
def test_rollout_is_the_hand_written_sequence_bit_for_bit_over_two_episodes(case):
    kw = CASES[case]
    cfg, engines, (ba, bb), actor, critic, vn = _setup(**kw)
    for ep in range(2):
        returns = policy.rollout(actor, critic, ba, vn)
        assert returns is ba.returns
        _by_hand(actor, critic, bb, vn, kw["cent"], kw["rnn"])
        _compare(ba, bb, "%s episode %d" % (case, ep))
        # the stored arrays are the policy's: values and states move, the done rows of the states are zero, the other rows are not
        vp, hs, hcs = ba.value_preds.cpu().numpy(), ba.rnn_states.cpu().numpy(), ba.rnn_states_critic.cpu().numpy()
        dn = ba.dones.bool().cpu().numpy()
        assert np.isfinite(vp).all() and np.unique(vp[:T]).size > T * ROWS // 2 and np.isfinite(ba.returns.cpu().numpy()).all()
        if kw["rnn"]:
            assert (hs[1:][dn] == 0).all() and (hcs[1:][dn] == 0).all()
            assert (np.abs(hs[1:][~dn]).max(axis=(-1, -2)) > 0).all() and (np.abs(hcs[1:][~dn]).max(axis=(-1, -2)) > 0).all()
        else:
            assert (hs == 0).all() and (hcs == 0).all()
        acts = ba.actions.cpu().numpy()[..., 0]
        assert (acts[1:][dn[:-1]] == K // 2).all() and (acts[1:][~dn[:-1]] != K // 2).any()
        for b in (ba, bb):
            b.after_update()
    assert ba.act_draw == 2 * T
    for e in engines:
        e.check_errors()
        e.close()


def test_rollout_is_collect_steps_then_compute_and_get_actions_returns_what_it_stores():
    cfg, engines, (ba, bb), actor, critic, vn = _setup(rnn=True, norm="valuenorm", cent=True)
    policy.rollout(actor, critic, ba, vn)
    for t in range(T):
        out = policy.collect_step(actor, critic, bb)
        assert out is engines[1].out and bb.step == (t + 1) % T
    assert policy.compute(critic, bb, vn) is bb.returns
    _compare(ba, bb, "rollout against collect_step + compute")
    # get_actions / get_values on a stored slot give the stored values, actions and log-probs again, in the reference's order and shapes
    t = 4
    s = policy._slot_rows(ba, t)
    values, actions, logp, h, hc = policy.get_actions(actor, critic, s["share_obs"], s["obs"], s["node_obs"], s["adj"], s["agent_id"], s["share_agent_id"],
                                                      s["rnn_states"], s["rnn_states_critic"], s["masks"], dones_prev=ba.dones[t - 1].view(ROWS),
                                                      seed=cfg.seed, env_id_base=cfg.env_id_base, num_agents=A, draw=t)
    slot = torch.zeros(ROWS, device=DEV)
    again = policy.get_values(critic, s["share_obs"], s["node_obs"], s["adj"], s["share_agent_id"], s["rnn_states_critic"], s["masks"], out=slot)
    torch.cuda.synchronize()
    assert [tuple(x.shape) for x in (values, actions, logp, h, hc)] == [(ROWS, 1), (ROWS, 1), (ROWS, 1), (ROWS, 1, 64), (ROWS, 1, 64)]
    assert actions.dtype == torch.int64 and not any(x.requires_grad for x in (values, logp, h, hc))
    _same(values.view(N, A, 1), ba.value_preds[t], "values")
    _same(actions.float().view(N, A, 1), ba.actions[t], "actions")
    _same(logp.view(N, A, 1), ba.action_log_probs[t], "action_log_probs")
    _same(again.view(N, A, 1), ba.value_preds[t], "get_values")
    assert again.data_ptr() == slot.data_ptr()
    live = ~ba.dones[t].bool().view(ROWS).cpu().numpy()
    assert np.array_equal(h.cpu().numpy()[live], ba.rnn_states[t + 1].reshape(ROWS, 1, 64).cpu().numpy()[live])
    for e in engines:
        e.check_errors()
        e.close()


def test_iteration_runs_twice_and_returns_finite_device_scalars():
    more = dict(clip_param=0.2, huber_delta=10.0, entropy_coef=0.01, use_policy_active_masks=True, use_value_active_masks=True,
                use_clipped_value_loss=True, use_huber_loss=True, use_max_grad_norm=True, max_grad_norm=0.5, value_loss_coef=0.5,
                use_recurrent_policy=True, use_naive_recurrent_policy=False, ppo_epoch=2, num_mini_batch=2, data_chunk_length=3)
    cfg, engines, (buf,), actor, critic, vn = _setup(rnn=True, norm="valuenorm", cent=True, buffers=1, **more)
    adam = lambda net: torch.optim.Adam(net.parameters(), lr=5e-4, eps=1e-5)
    aopt, copt = adam(actor), adam(critic)
    before = [p.detach().clone() for p in list(actor.parameters()) + list(critic.parameters())]
    infos = [policy.iteration(actor, critic, aopt, copt, buf, buf.args, vn, value_head=kind) for kind in ("torch", "device")]
    torch.cuda.synchronize()
    for info in infos:
        assert list(info) == list(policy.TRAIN_INFO) + ["average_episode_rewards"] and len(info) == 7
        for k, v in info.items():
            assert v.dim() == 0 and v.dtype == torch.float32 and v.device.type == "cuda" and not v.requires_grad and bool(torch.isfinite(v)), k
    assert buf.step == 0 and buf.act_draw == 2 * T
    _same(buf.obs[0], buf.obs[-1], "after_update carried the last slot")
    assert all(float(st["step"]) == 8 for opt in (aopt, copt) for st in opt.state.values())
    after = list(actor.parameters()) + list(critic.parameters())
    assert sum(not torch.equal(a, b) for a, b in zip(before, after)) > 40
    assert float(infos[0]["average_episode_rewards"]) != float(infos[1]["average_episode_rewards"])         # another episode
    engines[0].check_errors()
    engines[0].close()


@pytest.mark.parametrize("case", list(TL.TRAIN_CASES))
def test_train_with_the_device_value_head_ends_where_the_references_train_ends(case):
    fx = TL.load(case)
    train = lambda *a: policy.train(*a, value_head="device")
    info, got = TL.run_train(fx, train, DEV, torch.float32)
    torch.cuda.synchronize()
    worst = TL.compare(fx, info, got, TL.TRAIN_INFO, case + " value_head=device", TL.bound)
    print("%s value_head=device worst err_dev / bound %.3g" % (case, worst))
    assert "critic" in fx["meta"]                           # the critic's gradients, state and parameters are among what was compared
    # ... and the default path gives other bits in the critic: the keyword does select another v_out
    _, got_torch = TL.run_train(fx, policy.train, DEV, torch.float32)
    a, b = (TL.arrays_of(g["critic"], fx["meta"]["critic"])["param"] for g in (got, got_torch))
    print("%s critic param: max |device - torch| %.3g" % (case, float(np.abs(a - b).max())))
