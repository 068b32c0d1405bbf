"""The learner's fields of the device rollout buffer on the GPU (include/gmpe.h gmpe_insert_learner, DeviceRolloutBuffer learner_fields): the reference's own
buffer contents (tests/golden/learner_buffer_*.npz, made by tests/golden/make_learner_buffer_fixture.py) replayed through insert_external + after_update;
closed loops of two episodes on real engines against a plain-torch restatement of GMPERunner.insert on the engine's dones; caller storage as views of one
slab (16-byte and 4-byte paths of the kernel, strided slots); and the PPO generators drawing the buffer-owned fields."""
import glob
import os

import numpy as np
import pytest

import gmpe

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "learner_buffer_*.npz")))
FIELDS = ("rnn_states", "rnn_states_critic", "actions", "action_log_probs", "value_preds")


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def _same(a, b, what):
    import torch
    assert a.shape == b.shape and a.dtype == b.dtype == torch.float32, what
    assert torch.equal(_bits(a), _bits(b)), what


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_fixture_replay_is_the_reference_buffer_bit_for_bit(path):
    import torch
    from gmpe.engine import GmpeEngine
    from gmpe.rollout import DeviceRolloutBuffer
    d = np.load(path)
    T, N, A, R, H = (int(d[k]) for k in ("T", "N", "A", "R", "H"))
    cfg = gmpe.make_config(num_envs=N, num_agents=A, episode_length=T)
    eng = GmpeEngine(cfg, device=0)
    buf = DeviceRolloutBuffer(eng, T, use_centralized_V=bool(d["centralized"]), policy_fields=("value_preds",), learner_fields="all",
                              recurrent_N=R, hidden_size=H)
    buf.warmup()
    z = lambda x: torch.zeros_like(x[0])
    for t in range(T):
        buf.insert_external(z(buf.obs), z(buf.agent_id), z(buf._node_obs), z(buf._adj), z(buf.rewards), d["in_dones"][t],
                            values=d["in_values"][t].reshape(N * A, 1), actions=d["in_actions"][t].reshape(N * A, 1),
                            action_log_probs=d["in_action_log_probs"][t].reshape(N * A, 1), rnn_states=d["in_rnn_states"][t].reshape(N * A, R, H),
                            rnn_states_critic=d["in_rnn_states_critic"][t].reshape(N * A, R, H))
    assert buf.step == 0
    dev = eng.device
    for k in FIELDS:
        _same(getattr(buf, k), torch.as_tensor(d["buf_" + k], device=dev), k)
    buf.after_update()
    for k in FIELDS:
        _same(getattr(buf, k), torch.as_tensor(d["after_" + k], device=dev), "after_update " + k)
    eng.check_errors()
    eng.close()


C2_LIKE = dict(scenario_name="navigation_graph", num_agents=10, num_obstacles=0, num_walls=0, world_size=4.0)
ROT_INV = dict(scenario_name="nav_graph_metered_single_corridor_rot_inv", num_agents=4, num_obstacles=0, num_walls=0, world_size=2.4)


def _slab_storage(torch, spec, dev):
    """Every learner array as a view of ONE float32 slab, each starting 4 bytes past a 16-byte boundary: the kernel's 4-byte path and caller storage."""
    total = sum(int(np.prod(s)) + 8 for _, s in spec.values())
    slab = torch.full((total,), float("nan"), device=dev)
    out, off = {}, 1
    for name, (_, shape) in spec.items():
        n = int(np.prod(shape))
        out[name] = slab[off:off + n].view(shape).zero_()
        off += n + (4 - (off + n) % 4) + 1                                 # next view again 1 float past a 16-byte boundary
    return out


@pytest.mark.parametrize("kw, R, H, Hc", [(C2_LIKE, 1, 64, 64), (ROT_INV, 2, 6, 3)], ids=["c2like_R1_H64", "rotinv_R2_H6_Hc3"])
def test_closed_loop_two_episodes_match_a_torch_restatement(kw, R, H, Hc):
    """insert_step with the learner keywords on a real engine, two episodes of T steps with after_update between, against GMPERunner.insert restated with
    torch.where on the engine's own dones. A second engine (same config and actions: same dones) keeps its learner arrays in caller storage, as views of one
    slab at offsets that are not 16-byte aligned."""
    import torch
    from gmpe.engine import GmpeEngine
    from gmpe.rollout import DeviceRolloutBuffer, learner_storage_spec
    N, T = 48, 9
    cfg = gmpe.make_config(num_envs=N, episode_length=6, seed=11, **kw)        # time limit inside the rollout: whole-env dones
    A = cfg.num_agents
    engines = [GmpeEngine(cfg, device=0, adj_compact=True) for _ in range(2)]
    dev = engines[0].device
    spec = learner_storage_spec(cfg, T, recurrent_N=R, hidden_size=H, hidden_size_critic=Hc)
    storage = _slab_storage(torch, spec, dev)
    assert all(v.data_ptr() % 16 == 4 for v in storage.values())
    bufs = [DeviceRolloutBuffer(engines[0], T, policy_fields="all", learner_fields="all", recurrent_N=R, hidden_size=H, hidden_size_critic=Hc),
            DeviceRolloutBuffer(engines[1], T, policy_fields=("value_preds",), storage=storage, recurrent_N=R, hidden_size=H, hidden_size_critic=Hc)]
    for b in bufs:
        b.warmup()
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    want = {k: torch.zeros_like(getattr(bufs[0], k)) for k in FIELDS}
    for ep in range(2):
        for t in range(T):
            action = torch.randint(0, cfg.n_actions, (N * A, 1), generator=g, device=dev)        # int64, as the policy returns it
            vals = torch.randn((N * A, 1), generator=g, device=dev)
            logp = torch.randn((N * A, 1), generator=g, device=dev)
            rnn = torch.randn((N * A, R, H), generator=g, device=dev)
            rnn_c = torch.randn((N * A, R, Hc), generator=g, device=dev)
            for b in bufs:
                b.insert_step(action.view(N, A).to(torch.int32), values=vals, actions=action, action_log_probs=logp, rnn_states=rnn,
                              rnn_states_critic=rnn_c)
            done = bufs[0].dones[t].bool()
            want["value_preds"][t] = vals.view(N, A, 1)
            want["actions"][t] = action.view(N, A, 1).float()
            want["action_log_probs"][t] = logp.view(N, A, 1)
            want["rnn_states"][t + 1] = torch.where(done[:, :, None, None], torch.zeros((), device=dev), rnn.view(N, A, R, H))
            want["rnn_states_critic"][t + 1] = torch.where(done[:, :, None, None], torch.zeros((), device=dev), rnn_c.view(N, A, R, Hc))
        torch.cuda.synchronize()
        dn = bufs[0].dones.bool()
        assert torch.equal(dn, bufs[1].dones.bool())
        assert bool(dn.any()), "no agent was done in episode %d" % ep        # the time limit (6 < T) ends every env inside an episode
        for k in FIELDS:
            for i, b in enumerate(bufs):
                _same(getattr(b, k), want[k], "episode %d buffer %d %s" % (ep, i, k))
        for b in bufs:
            b.after_update()
        for k in ("rnn_states", "rnn_states_critic"):
            want[k][0] = want[k][-1]
        for i, b in enumerate(bufs):
            for k in FIELDS:
                _same(getattr(b, k), want[k], "after_update %d buffer %d %s" % (ep, i, k))
    for e in engines:
        e.check_errors()
        e.close()


def test_insert_learner_at_strided_slots_and_odd_rows():
    """gmpe.engine.insert_learner directly: slots stride(0) elements apart with a gap (views into wider rows), row lengths that are and are not multiples of
    4 floats, odd lane counts, float32 actions, one field at a time, against torch.where."""
    import torch
    from gmpe.engine import insert_learner
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    for (T, N, A, R, H, k) in ((4, 7, 3, 1, 64, 1), (3, 33, 5, 3, 5, 2), (2, 1, 1, 1, 1, 1), (5, 257, 10, 2, 32, 1)):
        lanes = N * A
        slot = lambda *tail: lanes * int(np.prod(tail))
        wide = lambda S, *tail: torch.full((S, slot(*tail) + 12), 7.0, device=dev)[:, 4:4 + slot(*tail)].view(S, N, A, *tail)
        arrays = dict(value_preds=wide(T + 1, 1), actions=wide(T, k), action_log_probs=wide(T, k), rnn_states=wide(T + 1, R, H),
                      rnn_states_critic=wide(T + 1, R, H + 1))
        before = {n: v.clone() for n, v in arrays.items()}
        dones = (torch.rand((T, N, A), generator=g, device=dev) < 0.4).to(torch.uint8)
        for t in range(T):
            ins = dict(values=torch.randn((lanes, 1), generator=g, device=dev), actions=torch.randn((lanes, k), generator=g, device=dev),
                       action_log_probs=torch.randn((lanes, k), generator=g, device=dev), rnn_states=torch.randn((lanes, R, H), generator=g, device=dev),
                       rnn_states_critic=torch.randn((lanes, R, H + 1), generator=g, device=dev))
            if t == 1:
                insert_learner(t, dones, arrays, rnn_states=ins["rnn_states"])            # one field: the others keep what they hold
                before["rnn_states"][t + 1] = torch.where(dones[t].bool()[:, :, None, None], torch.zeros((), device=dev), ins["rnn_states"].view(N, A, R, H))
                continue
            insert_learner(t, dones, arrays, **ins)
            dn = dones[t].bool()
            before["value_preds"][t] = ins["values"].view(N, A, 1)
            before["actions"][t] = ins["actions"].view(N, A, k)
            before["action_log_probs"][t] = ins["action_log_probs"].view(N, A, k)
            for n in ("rnn_states", "rnn_states_critic"):
                x = ins[n].view(N, A, R, -1)
                before[n][t + 1] = torch.where(dn[:, :, None, None], torch.zeros((), device=dev), x)
        torch.cuda.synchronize()
        for n in arrays:
            _same(arrays[n], before[n], "T=%d N=%d A=%d R=%d H=%d k=%d %s" % (T, N, A, R, H, k, n))
            base = arrays[n]._base if arrays[n]._base is not None else arrays[n]
            assert float(base.view(arrays[n].shape[0], -1)[:, :4].min()) == 7.0 == float(base.view(arrays[n].shape[0], -1)[:, -8:].max())   # gaps untouched


def test_generators_draw_the_buffer_owned_learner_fields():
    """feed_forward_generator / recurrent_generator with learner=None on a buffer that keeps its learner fields == the same generators with those tensors
    passed as learner=; the learner slots of the 16-tuple (rnn_states, rnn_states_critic, actions, action_log_probs) are not None."""
    import torch
    from gmpe.engine import GmpeEngine
    from gmpe.minibatch import TUPLE
    from gmpe.rollout import LEARNER_FIELDS, DeviceRolloutBuffer
    N, A, T, L, R, H = 24, 3, 8, 4, 2, 16
    cfg = gmpe.make_config(num_envs=N, num_agents=A, episode_length=5, seed=2)
    eng = GmpeEngine(cfg, device=0)
    buf = DeviceRolloutBuffer(eng, T, policy_fields="all", learner_fields="all", recurrent_N=R, hidden_size=H)
    buf.warmup()
    dev = eng.device
    g = torch.Generator(device=dev)
    g.manual_seed(9)
    for t in range(T):
        action = torch.randint(0, cfg.n_actions, (N * A, 1), generator=g, device=dev)
        buf.insert_step(action.view(N, A).to(torch.int32), values=torch.randn((N * A, 1), generator=g, device=dev), actions=action,
                        action_log_probs=torch.randn((N * A, 1), generator=g, device=dev), rnn_states=torch.randn((N * A, R, H), generator=g, device=dev),
                        rnn_states_critic=torch.randn((N * A, R, H), generator=g, device=dev))
    adv = torch.randn((T, N, A, 1), generator=g, device=dev)
    learner = {k: getattr(buf, k).clone() for k in LEARNER_FIELDS}
    perm_ff = torch.randperm(T * N * A, generator=g, device=dev)
    perm_rec = torch.randperm(T * N * A // L, generator=g, device=dev)
    own = (list(buf.feed_forward_generator(adv, 4, perm=perm_ff)), list(buf.recurrent_generator(adv, 3, L, perm=perm_rec)))
    given = (list(buf.feed_forward_generator(adv, 4, learner=learner, perm=perm_ff)), list(buf.recurrent_generator(adv, 3, L, learner=learner, perm=perm_rec)))
    torch.cuda.synchronize()
    for kind, a, b in zip(("feed_forward", "recurrent"), own, given):
        assert len(a) == len(b) > 0
        for i, (x, y) in enumerate(zip(a, b)):
            assert len(x) == len(y) == 16
            for name, u, v in zip(TUPLE, x, y):
                assert (u is None) == (v is None), (kind, i, name)
                if name in LEARNER_FIELDS:
                    assert u is not None, (kind, i, name)
                if u is not None:
                    assert u.dtype == v.dtype and torch.equal(u, v), (kind, i, name)
    # an explicit learner array still overrides the buffer's own
    other = dict(actions=learner["actions"] + 1.0)
    mb = next(iter(buf.feed_forward_generator(adv, 4, learner=other, perm=perm_ff)))
    ref = next(iter(buf.feed_forward_generator(adv, 4, perm=perm_ff)))
    i = TUPLE.index("actions")
    assert torch.equal(mb[i], ref[i] + 1.0)
    eng.check_errors()
    eng.close()
