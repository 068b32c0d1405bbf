"""gmpe.policy.CapturedUpdate — one ppo_update captured as a graph and replayed — against the eager gmpe.policy.ppo_update / train on twin networks
and optimisers, bit for bit: a replay launches the same kernels on the same inputs in the same order, and nothing on this path uses atomics, so
equality is the expectation, not a tolerance. The networks are tests/test_gpu_policy.py's _Net with tests/test_gpu_ppo_update.py's PopArt critic (the
device loss's duck-typed PopArt) and tests/trainer_lib.py's ValueNorm; the samples come from a DeviceRolloutBuffer over 4 envs x 3 agents, built as
tests/test_gpu_optim_shards.py::_buffer builds it: 24 rows per recurrent minibatch (chunks of 2), 48 per feed-forward one."""
import functools
import types

import numpy as np
import pytest
import torch

import gmpe
import gnn_lib as G
import head_lib as HL
from gmpe import policy
from test_gpu_policy import DEV, K, _Net, same
from test_gpu_ppo_update import EPS, LR, _Critic, update_args
from trainer_lib import ValueNorm

pytestmark = pytest.mark.gpu
N, A = 4, 3
FLAVOURS = ("plain", "valuenorm", "popart")
NORM_TENSORS = ("running_mean", "running_mean_sq", "debiasing_term", "weight", "bias", "stddev", "mean", "mean_sq")


def _buffer(seed, T):
    from gmpe.engine import GmpeEngine
    from gmpe.rollout import DeviceRolloutBuffer
    cfg = gmpe.make_config(num_envs=N, num_agents=A, episode_length=5, seed=seed)
    eng = GmpeEngine(cfg, device=0)
    bargs = types.SimpleNamespace(gamma=0.99, gae_lambda=0.95, use_gae=True, use_proper_time_limits=False, use_valuenorm=False, use_popart=False)
    buf = DeviceRolloutBuffer(eng, T, use_centralized_V=False, policy_fields="all", learner_fields="all", args=bargs, recurrent_N=1, hidden_size=64)
    buf.warmup()
    g = torch.Generator(device=DEV)
    g.manual_seed(seed + 4)
    for t in range(T):
        logits = torch.randn((N * A, int(cfg.n_actions)), generator=g, device=DEV)
        vals = torch.randn((N * A, 1), generator=g, device=DEV)
        rnn = torch.rand((N * A, 1, 64), generator=g, device=DEV) * 2 - 1
        buf.act_step(logits, vals, rnn_states=rnn, rnn_states_critic=rnn)
    buf.compute_returns(torch.randn((N, A, 1), generator=g, device=DEV))
    return cfg, eng, buf


@functools.lru_cache(maxsize=None)
def world(T):
    """one buffer of T steps for every test that reads it: (cfg, engine, buffer, the GNN key, obs_dim); nothing writes to it afterwards"""
    cfg, eng, buf = _buffer(13, T)
    key = G.ACTOR if int(cfg.node_feats) == 7 else G.ROTATE
    assert G.CONFIGS[key]["F"] == int(cfg.node_feats) and int(cfg.n_actions) == K
    return cfg, eng, buf, key, eng.D


@functools.lru_cache(maxsize=None)
def samples(recurrent):
    """three different minibatches of the four-step buffer: 24 rows in chunks of 2, or 48 rows"""
    _, _, buf, _, _ = world(4)
    adv = buf.normalized_advantages(None)
    g = torch.Generator().manual_seed(5)
    out = []
    for _ in range(3 if not recurrent else 2):
        perm = torch.randperm(24 if recurrent else 48, generator=g).to(DEV)
        gen = buf.recurrent_generator(adv, 2, 2, perm=perm) if recurrent else buf.feed_forward_generator(adv, 1, perm=perm)
        out += [tuple(None if t is None else t.clone() for t in s) for s in gen]
    out = out[:3]
    assert [int(s[1].shape[0]) for s in out] == [24 if recurrent else 48] * 3
    assert not same(out[0][1], out[1][1]) and not same(out[1][1], out[2][1])
    return out


def build(flavour, T=4):
    """(actor, critic, actor_optimizer, critic_optimizer, value_normalizer, args): two calls give twins"""
    _, _, _, key, D = world(T)
    actor = _Net(key, D, "act").to(DEV)
    critic = _Critic(key, D, "popart" if flavour == "popart" else "v_out", seed=12).to(DEV)
    if flavour == "popart":
        critic.v_out = HL.PopArt(DEV)
    adam = lambda net: torch.optim.Adam(list(net.parameters()), lr=LR, eps=EPS, weight_decay=0)
    args = update_args(max_grad_norm=0.5, use_popart=flavour == "popart", use_valuenorm=flavour == "valuenorm")
    return actor, critic, adam(actor), adam(critic), ValueNorm(DEV) if flavour == "valuenorm" else None, args


def everything(actor, critic, aopt, copt, vn, grads=False):
    """every parameter, Adam moment and host step count, every ValueNorm / PopArt tensor, and with grads every .grad (None where there is none)"""
    out = {"actor." + k: p for k, p in actor.named_parameters()}
    out.update({"critic." + k: p for k, p in critic.named_parameters()})
    for tag, o in (("vn.", vn), ("v_out.", critic.v_out)):
        if o is not None:
            out.update({tag + k: getattr(o, k) for k in NORM_TENSORS if isinstance(getattr(o, k, None), torch.Tensor)})
    for tag, opt in (("aopt", aopt), ("copt", copt)):
        for i, p in enumerate(p for g in opt.param_groups for p in g["params"]):
            out["%s.%d" % (tag, i)] = p
            for k, v in opt.state.get(p, {}).items():
                out["%s.%d.%s" % (tag, i, k)] = v
            if grads:
                out["%s.%d.grad" % (tag, i)] = p.grad
    return {k: None if v is None else v.detach().cpu().numpy().copy() for k, v in out.items()}


def equal_dicts(a, b, what=""):
    assert sorted(a) == sorted(b), (what, sorted(set(a) ^ set(b)))
    for k in a:
        assert (a[k] is None) == (b[k] is None) and (a[k] is None or same(a[k], b[k])), (what, k)


def equal_updates(ua, ub, what):
    assert isinstance(ub, policy.PPOUpdate) and ub._fields == ua._fields and len(ua._fields) == 7
    for k in ua._fields:
        x, y = getattr(ua, k), getattr(ub, k)
        assert x.dtype == y.dtype == torch.float32 and x.shape == y.shape and same(x, y), (what, k, x, y)


@pytest.mark.parametrize("recurrent", [True, False], ids=["recurrent-24", "feed-forward-48"])
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_three_replays_are_three_eager_updates_bit_for_bit(flavour, recurrent):
    ss = samples(recurrent)
    a, b = build(flavour), build(flavour)
    cap = policy.CapturedUpdate(*b[:4], ss[0], b[5], b[4], steps_ahead=8)
    assert cap.remaining == 8
    start = everything(*a[:5])
    for i, s in enumerate(ss):
        ua = policy.ppo_update(*a[:4], s, a[5], a[4], install="in_place")
        ub = cap.update(s)
        equal_updates(ua, ub, "update %d" % i)
        assert float(ub.actor_grad_norm) > 0 and float(ub.critic_grad_norm) > 0 and tuple(ub.imp_weights.shape) == (s[1].shape[0], 1)
        equal_dicts(everything(*a[:5]), everything(*b[:5]), "after update %d" % i)
    assert cap.remaining == 5
    got = everything(*b[:5])
    assert sum(not same(start[k], got[k]) for k in start if k.startswith(("actor.", "critic."))) > 40
    assert all(float(st["step"]) == 3 for opt in (b[2], b[3]) for st in opt.state.values() if st)
    if flavour != "plain":
        norm = "vn.running_mean" if flavour == "valuenorm" else "v_out.mean"
        assert not same(got[norm], np.zeros(1, np.float32))                 # the normaliser moved, three times, as in the eager run
    # eager takes over from the state the replays left
    ua, ub = policy.ppo_update(*a[:4], ss[0], a[5], a[4], install="in_place"), policy.ppo_update(*b[:4], ss[0], b[5], b[4], install="in_place")
    equal_updates(ua, ub, "eager after the replays")
    equal_dicts(everything(*a[:5]), everything(*b[:5]), "eager after the replays")
    with pytest.raises(ValueError, match=r"sample\[0\] must be"):
        cap.update(samples(not recurrent)[0])


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_construction_leaves_every_tensor_as_it_found_it(flavour):
    ss = samples(True)
    # from a trained state: gradients, moments and counts are there, and stay, to the object
    nets = build(flavour)
    policy.ppo_update(*nets[:4], ss[1], nets[5], nets[4], install="in_place")
    before = everything(*nets[:5], grads=True)
    grad_objects = [p.grad for opt in nets[2:4] for g in opt.param_groups for p in g["params"]]
    assert sum(g is not None for g in grad_objects) > 40
    cap = policy.CapturedUpdate(*nets[:4], ss[0], nets[5], nets[4])
    torch.cuda.synchronize()
    equal_dicts(before, everything(*nets[:5], grads=True), "construction over a trained state")
    assert all(p.grad is g for p, g in zip((p for opt in nets[2:4] for g in opt.param_groups for p in g["params"]), grad_objects))
    assert cap.remaining == gmpe.optim.STEPS_AHEAD and int(cap.critic_step.counter) == 0 and int(cap.actor_step.counter) == 0
    # from a fresh state: parameters and normaliser as before; the new Adam state is torch's (zeros, step 0) and the new gradients are zero
    fresh = build(flavour)
    before = everything(*fresh[:5])
    policy.CapturedUpdate(*fresh[:4], ss[0], fresh[5], fresh[4], steps_ahead=2)
    after = everything(*fresh[:5], grads=True)
    for k, v in before.items():
        assert same(v, after[k]), k
    new = [k for k in after if k not in before]
    assert len(new) > 160 and all(after[k] is None or not after[k].any() for k in new), [k for k in new if after[k] is not None and after[k].any()][:5]


def test_without_update_actor_the_actor_keeps_its_bits():
    ss = samples(True)
    a, b = build("plain"), build("plain")
    before = everything(*b[:5])
    cap = policy.CapturedUpdate(*b[:4], ss[0], b[5], None, update_actor=False, steps_ahead=4)
    assert cap.actor_step is None
    for i, s in enumerate(ss[:2]):
        ua = policy.ppo_update(*a[:4], s, a[5], None, update_actor=False, install="in_place")
        ub = cap.update(s)
        equal_updates(ua, ub, "update %d" % i)
        assert float(ub.actor_grad_norm) == 0.0 and float(ub.critic_grad_norm) > 0
    after = everything(*b[:5])
    assert not any(b[2].state.values())
    for k in before:
        if k.startswith(("actor.", "aopt.")):
            assert same(before[k], after[k]), k
    assert any(not same(before[k], after[k]) for k in before if k.startswith("critic."))
    equal_dicts(everything(*a[:5]), after)


@pytest.mark.parametrize("recurrent", [True, False], ids=["recurrent", "feed-forward"])
def test_train_is_policy_train_bit_for_bit(recurrent):
    _, eng, buf, _, _ = world(2)
    a, b = build("plain", T=2), build("plain", T=2)
    args = a[5]
    args.ppo_epoch, args.num_mini_batch, args.data_chunk_length = 2, 2, 2
    args.use_recurrent_policy, args.use_naive_recurrent_policy = recurrent, False
    for k in ("ppo_epoch", "num_mini_batch", "data_chunk_length", "use_recurrent_policy", "use_naive_recurrent_policy"):
        setattr(b[5], k, getattr(args, k))
    g = torch.Generator().manual_seed(23)
    perms = [torch.randperm(12 if recurrent else 24, generator=g).to(DEV) for _ in range(2)]
    adv = buf.normalized_advantages(None)
    first = next(iter(buf.recurrent_generator(adv, 2, 2, perm=perms[0]) if recurrent else buf.feed_forward_generator(adv, 2, perm=perms[0])))
    assert int(first[1].shape[0]) == 12
    cap = policy.CapturedUpdate(*b[:4], first, b[5], None, steps_ahead=4)
    want = policy.train(*a[:4], buf, args, perms=perms, install="in_place")
    got = cap.train(buf, perms=perms)
    assert list(got) == list(policy.TRAIN_INFO) == list(want)
    for k in want:
        assert got[k].dim() == 0 and got[k].dtype == torch.float32 and bool(torch.isfinite(got[k])) and same(got[k], want[k]), k
    equal_dicts(everything(*a[:5]), everything(*b[:5]))
    assert all(float(st["step"]) == 4 for opt in b[2:4] for st in opt.state.values() if st) and cap.remaining == 0
    # a second pass: the schedules are spent, train refills them by itself, from the optimisers' counts and a decayed lr
    for x in (a, b):
        for opt in x[2:4]:
            opt.param_groups[0]["lr"] = LR / 2
    want = policy.train(*a[:4], buf, args, perms=perms, install="in_place")
    got = cap.train(buf, perms=perms)
    for k in want:
        assert same(got[k], want[k]), k
    equal_dicts(everything(*a[:5]), everything(*b[:5]))
    with pytest.raises(ValueError, match="one permutation per epoch"):
        cap.train(buf, perms=perms[:1])
    with pytest.raises(RuntimeError, match="CapturedUpdate.update: the schedule holds 4 steps and 4 are used"):
        cap.update(first)
    eng.check_errors()


def test_a_replay_waits_for_nothing():
    """torch's sync debug mode raises at every call that waits for the device; a deliberate .item() shows that this build honours it"""
    ss = samples(True)
    nets = build("valuenorm")
    cap = policy.CapturedUpdate(*nets[:4], ss[0], nets[5], nets[4], steps_ahead=4)
    cap.update(ss[0])
    one = torch.ones((), device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            one.item()
        u = cap.update(ss[1])
        u = cap.update(ss[2])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(u.value_loss)) and cap.remaining == 1
