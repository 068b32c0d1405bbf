"""DeviceRolloutBuffer.act_step — the action head inside the closed loop's launch sequence — against the sequence it replaces, written by hand from the
buffer's existing methods: available_actions_for + gmpe.sample_actions + insert_step(actions=..., action_log_probs=...). Every array of the two buffers
must agree bit for bit over two episodes with dones in them."""
import numpy as np
import pytest

import gmpe

pytestmark = pytest.mark.gpu
N, A, T = 8, 3, 9
ARRAYS = ("obs", "agent_id", "rewards", "dones", "masks", "active_masks", "value_preds", "available_actions", "actions", "action_log_probs", "rnn_states",
          "rnn_states_critic", "_adj", "_node_obs")


def _buffers(torch, *kws):
    """One engine (the same config: the same envs) and one warmed-up buffer per keyword dict."""
    from gmpe.engine import GmpeEngine
    from gmpe.rollout import DeviceRolloutBuffer
    cfg = gmpe.make_config(num_envs=N, num_agents=A, episode_length=6, seed=11)   # the time limit lies inside the rollout: dones occur
    engines = [GmpeEngine(cfg, device=0) for _ in kws]
    bufs = [DeviceRolloutBuffer(e, T, recurrent_N=1, hidden_size=8, **kw) for e, kw in zip(engines, kws)]
    for b in bufs:
        b.warmup()
    return cfg, engines, bufs


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert np.array_equal(a.cpu().numpy().view(np.uint8), b.cpu().numpy().view(np.uint8)), what


def test_act_step_equals_the_hand_written_sequence_over_two_episodes():
    import torch
    cfg, engines, (ba, bh) = _buffers(torch, *[dict(policy_fields="all", learner_fields="all")] * 2)
    K, dev = cfg.n_actions, engines[0].device
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    assert ba.act_draw == 0
    draw = 0
    for ep in range(2):
        for t in range(T):
            logits = torch.randn((N * A, K), generator=g, device=dev) * 2.0
            vals = torch.randn((N * A, 1), generator=g, device=dev)
            rnn = torch.randn((N * A, 1, 8), generator=g, device=dev)
            ba.act_step(logits, vals, rnn_states=rnn, rnn_states_critic=rnn)
            avail = bh.available_actions_for(t)
            idx, act, logp = gmpe.sample_actions(logits, avail.view(N * A, K), seed=cfg.seed, env_id_base=cfg.env_id_base, num_agents=A, draw=draw)
            bh.insert_step(idx.view(N, A), vals, actions=act, action_log_probs=logp, rnn_states=rnn, rnn_states_critic=rnn)
            draw += 1
            assert ba.act_draw == draw and ba.step == bh.step
        torch.cuda.synchronize()
        dn = ba.dones.bool().cpu().numpy()
        assert dn.any() and not dn.all(), "episode %d: dones %d" % (ep, dn.sum())
        for k in ARRAYS:
            x, y = getattr(ba, k), getattr(bh, k)
            assert (x is None) == (y is None), k
            if x is not None:
                _same(x, y, "episode %d %s" % (ep, k))
        # after a done, the agent's next stored action is the stop action with log-prob +0; elsewhere other actions occur
        acts, lps = ba.actions.cpu().numpy()[..., 0], ba.action_log_probs.cpu().numpy()[..., 0]
        after = dn[:-1]
        assert after.any()
        assert (acts[1:][after] == K // 2).all() and (lps[1:][after].view(np.int32) == 0).all()
        assert (acts[1:][~after] != K // 2).any() and (acts == np.floor(acts)).all() and acts.min() >= 0 and acts.max() < K
        assert (ba.available_actions.cpu().numpy()[np.arange(1, T + 1)[:, None, None], np.arange(N)[None, :, None], np.arange(A)[None, None, :],
                                                   acts.astype(np.int64)] == 1.0).all()
        for b in (ba, bh):
            b.after_update()
    for e in engines:
        e.check_errors()
        e.close()


def test_act_step_without_the_optional_fields_deterministic_and_carried():
    """A buffer that keeps none of the policy's arrays still acts (the log-probs go to scratch the buffer owns) and takes the same actions, which shows in
    the env's own outputs; deterministic=True takes the mode; carry_from hands the draw counter on; a buffer without value_preds refuses values."""
    import torch
    from gmpe.rollout import DeviceRolloutBuffer
    cfg, engines, (full, bare, det) = _buffers(torch, dict(learner_fields=("actions", "action_log_probs")), {}, {})
    K, dev = cfg.n_actions, engines[0].device
    g = torch.Generator(device=dev)
    g.manual_seed(4)
    with pytest.raises(ValueError, match="value_preds"):
        bare.act_step(torch.zeros(N * A, K, device=dev), torch.zeros(N * A, 1, device=dev))
    with pytest.raises(ValueError, match="logits must be a tensor of shape"):
        bare.act_step(torch.zeros(N * A, K + 1, device=dev))
    assert bare.act_draw == 0 and bare.step == 0
    modes = []
    for t in range(T):
        logits = torch.randn((N * A, K), generator=g, device=dev) * 2.0
        full.act_step(logits)
        bare.act_step(logits)
        det.act_step(logits, deterministic=True)
        prev = det.dones[t - 1].bool().view(-1) if t else torch.zeros(N * A, dtype=torch.bool, device=dev)
        want = torch.where(prev, torch.full_like(prev, K // 2, dtype=torch.int32), logits.argmax(dim=1).to(torch.int32))
        modes.append(bool(torch.equal(det._act_idx.view(-1), want)))
    torch.cuda.synchronize()
    assert all(modes)
    for k in ("obs", "rewards", "dones", "masks", "active_masks"):
        _same(getattr(full, k), getattr(bare, k), k)
    assert bare.actions is None and bare.action_log_probs is None and full.act_draw == bare.act_draw == T
    nxt = DeviceRolloutBuffer(engines[0], T)
    nxt.carry_from(full)
    assert nxt.act_draw == T and nxt.step == 0
    for e in engines:
        e.check_errors()
        e.close()
