"""gmpe.policy.ppo_update and gmpe.policy.train — GR_MAPPO.ppo_update / train composed from minibatch_losses and clip_and_step — at the shapes of
tests/test_gpu_policy.py (6 x 5 rows, E = 7, K = 25). The composition adds no arithmetic, so it is compared bit for bit with the same sequence written
out by hand; the step itself is held to the accuracy rule against the float64 restatement applied to the device's own gradients (err_ref from torch's
float32 clip + Adam on the CPU on those gradients); train runs under torch's sync debug mode, where any wait for the device raises."""
import types

import numpy as np
import pytest
import torch

import gmpe
import gnn_lib as G
import head_lib as HL
import optim_lib as OL
from gmpe import policy
from test_gpu_policy import DEV, K, OBS, _Net, loss_args, same, sample_of

pytestmark = pytest.mark.gpu
LR, EPS = 5e-4, 1e-5


class _Critic(_Net):
    """a critic whose parameters() reach a PopArt v_out's weight and bias, as the reference's PopArt (an nn.Module) lets them"""

    def parameters(self, recurse=True):
        for p in super().parameters(recurse):
            yield p
        if isinstance(getattr(self, "v_out", None), HL.PopArt):
            yield self.v_out.weight
            yield self.v_out.bias


def nets(popart=False):
    actor = _Net(G.ACTOR, OBS, "act").to(DEV)
    critic = _Critic(G.CRITIC, OBS, "popart" if popart else "v_out", seed=12).to(DEV)
    if popart:
        critic.v_out = HL.PopArt(DEV)
    adam = lambda net: torch.optim.Adam(list(net.parameters()), lr=LR, eps=EPS, weight_decay=0)
    return actor, critic, adam(actor), adam(critic)


def update_args(**over):
    kw = dict(use_max_grad_norm=True, max_grad_norm=0.01, value_loss_coef=0.5)
    kw.update(over)
    a = loss_args(**{k: kw.pop(k) for k in list(kw) if k in ("use_popart", "use_valuenorm")})
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def by_hand(actor, critic, aopt, copt, s, args, update_actor=True, install="replace", seen=None):
    """ppo_update's sequence (graph_mappo.py:202-271) written out; seen: a dict that receives the critic optimiser's gradients before the clip"""
    res = policy.minibatch_losses(actor, critic, s, args, install=install)
    aopt.zero_grad()
    if update_actor:
        res.actor_loss.backward()
    an = gmpe.clip_and_step(aopt, args.max_grad_norm, parameters=actor.parameters(), step=update_actor)
    copt.zero_grad()
    (res.value_loss * args.value_loss_coef).backward()
    if seen is not None:
        seen.update({id(p): p.grad.clone() for g in copt.param_groups for p in g["params"] if p.grad is not None})
    cn = gmpe.clip_and_step(copt, args.max_grad_norm, parameters=critic.parameters())
    return policy.PPOUpdate(res.value_loss.detach(), cn, res.policy_loss.detach(), res.dist_entropy.detach(), an, res.ratio_mean.detach(),
                            res.imp_weights.detach())


def everything(actor, critic, aopt, copt):
    """every parameter and every state tensor, by name"""
    out = {"actor." + k: p for k, p in actor.named_parameters()}
    out.update({"critic." + k: p for k, p in critic.named_parameters()})
    if isinstance(critic.v_out, HL.PopArt):
        out.update({"critic.v_out." + k: getattr(critic.v_out, k) for k in ("weight", "bias", "stddev")})
    for tag, opt in (("aopt", aopt), ("copt", copt)):
        i = 0
        for g in opt.param_groups:
            for p in g["params"]:
                out["%s.%d" % (tag, i)] = p
                for k, v in opt.state.get(p, {}).items():
                    out["%s.%d.%s" % (tag, i, k)] = v
                i += 1
    return {k: v.detach().cpu().numpy().copy() for k, v in out.items()}


def equal_dicts(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert same(a[k], b[k]), k


@pytest.mark.parametrize("case", ["plain", "popart-replace", "popart-in_place"])
def test_ppo_update_is_the_hand_written_sequence_bit_for_bit(case):
    popart = case != "plain"
    install = "in_place" if case.endswith("in_place") else "replace"
    s, args = sample_of(), update_args(use_popart=popart)
    runs = []
    for fn in (policy.ppo_update, by_hand):
        actor, critic, aopt, copt = nets(popart)
        before = everything(actor, critic, aopt, copt)
        old = [critic.v_out.weight, critic.v_out.bias] if popart else []
        seen = {}
        u = fn(actor, critic, aopt, copt, s, args, install=install, **({"seen": seen} if fn is by_hand else {}))
        torch.cuda.synchronize()
        after = everything(actor, critic, aopt, copt)
        runs.append((u, after))
        assert isinstance(u, policy.PPOUpdate) and tuple(u.imp_weights.shape) == (s[1].shape[0], 1)
        for k in u._fields[:6]:
            t = getattr(u, k)
            assert t.dim() == 0 and t.dtype == torch.float32 and t.device.type == "cuda" and not t.requires_grad and bool(torch.isfinite(t)), k
        assert float(u.actor_grad_norm) > args.max_grad_norm and float(u.critic_grad_norm) > args.max_grad_norm       # both clips bite
        changed = [k for k in before if k in after and not same(before[k], after[k])]
        assert any(k.startswith("actor.") for k in changed) and any(k.startswith("critic.") for k in changed)
        assert all(float(st["step"]) == 1 for opt in (aopt, copt) for st in opt.state.values() if st)
        if popart and install == "replace":
            # the optimiser holds the old v_out objects: stepped, with their gradients as backward left them (the clip ran over critic.parameters(), which
            # holds the new ones); the new ones have no gradient, no state, and the bits the PopArt update gave them
            assert critic.v_out.weight is not old[0] and critic.v_out.bias is not old[1]
            for p in old:
                assert p in copt.state and float(copt.state[p]["step"]) == 1 and p.grad is not None
                if fn is by_hand:
                    assert same(p.grad, seen[id(p)])
            assert not same(old[0], before["critic.v_out.weight"])
            for p in (critic.v_out.weight, critic.v_out.bias):
                assert p.grad is None and p not in copt.state
            if fn is by_hand:                            # every other gradient of the critic was scaled
                scaled = [p for g in copt.param_groups for p in g["params"] if p.grad is not None and all(p is not q for q in old)]
                assert scaled and all(not same(p.grad, seen[id(p)]) for p in scaled if float(seen[id(p)].abs().max()) > 0)
        elif popart:
            assert critic.v_out.weight is old[0] and old[0] in copt.state and not same(old[0], before["critic.v_out.weight"])
    (ua, aa), (ub, ab) = runs
    equal_dicts(aa, ab)
    for k in ua._fields:
        assert same(getattr(ua, k), getattr(ub, k)), k


def test_without_update_actor_the_actor_keeps_its_bits():
    s, args = sample_of(), update_args()
    actor, critic, aopt, copt = nets()
    before = everything(actor, critic, aopt, copt)
    u = policy.ppo_update(actor, critic, aopt, copt, s, args, update_actor=False)
    after = everything(actor, critic, aopt, copt)
    assert float(u.actor_grad_norm) == 0.0 and u.actor_grad_norm.dtype == torch.float32 and float(u.critic_grad_norm) > 0
    assert len(aopt.state) == 0 and all(p.grad is None for p in actor.parameters())
    for k in before:
        if k.startswith("actor.") or k.startswith("aopt."):
            assert same(before[k], after[k]), k
    assert any(not same(before[k], after[k]) for k in before if k.startswith("critic."))
    # without use_max_grad_norm the norm is only reported: the gradients keep the bits backward gave them
    actor, critic, aopt, copt = nets()
    args = update_args(use_max_grad_norm=False)
    res = policy.minibatch_losses(actor, critic, s, args)
    res.actor_loss.backward()
    raw = [p.grad.clone() for p in actor.parameters()]
    actor.zero_grad()
    u = policy.ppo_update(actor, critic, aopt, copt, s, args)
    assert all(same(p.grad, g) for p, g in zip(actor.parameters(), raw))
    want = np.sqrt(sum(float((g.double() ** 2).sum()) for g in raw))
    assert abs(float(u.actor_grad_norm) - want) <= 2.0 ** -22 * want


@pytest.mark.parametrize("which", ["actor", "critic"])
def test_the_step_meets_the_accuracy_rule_on_the_devices_own_gradients(which):
    s, args = sample_of(), update_args()
    actor, critic, aopt, copt = nets()
    net, opt = (actor, aopt) if which == "actor" else (critic, copt)
    names = [k for k, _ in net.named_parameters()]
    params = [p.detach().cpu().numpy().copy() for p in net.parameters()]
    res = policy.minibatch_losses(actor, critic, s, args)
    (res.actor_loss if which == "actor" else res.value_loss * args.value_loss_coef).backward()
    grads = [p.grad.detach().cpu().numpy().copy() for p in net.parameters()]
    norm = gmpe.clip_and_step(opt, args.max_grad_norm, parameters=net.parameters())
    torch.cuda.synchronize()
    # torch on the CPU in float32, and the restatement, on those gradients
    rps = OL.torch_params(params)
    ropt = torch.optim.Adam(rps, lr=LR, eps=EPS, weight_decay=0)
    OL.set_grads(rps, grads)
    rnorm = torch.nn.utils.clip_grad_norm_(rps, args.max_grad_norm)
    ropt.step()
    r = OL.Restated(params)
    tnorm, tg = r.step(grads, args.max_grad_norm, lr=LR, eps=EPS)
    assert tnorm > args.max_grad_norm and len(names) >= 40
    dev = OL.snapshot(list(net.parameters()), opt, norm)
    ref = OL.snapshot(rps, ropt, rnorm)
    truth = {"param": r.p, "grad": tg, "exp_avg": r.m, "exp_avg_sq": r.v, "norm": tnorm}
    e_dev, e_ref = OL.errors(dev, truth), OL.errors(ref, truth)
    for k in e_dev:
        print("%s %-10s err_ref %.3g err_dev %.3g bound %.3g" % (which, k, e_ref[k], e_dev[k], OL.bound(e_ref[k])))
    for k in e_dev:
        assert e_ref[k] <= OL.CAP and e_dev[k] <= OL.bound(e_ref[k]), (which, k, e_dev[k], e_ref[k])


# ---------------------------------------------------------------------------------------------- train
N, A, T = 4, 3, 8


def _buffer():
    from gmpe.engine import GmpeEngine
    from gmpe.rollout import DeviceRolloutBuffer
    cfg = gmpe.make_config(num_envs=N, num_agents=A, episode_length=5, seed=13)       # the time limit lies inside the rollout: dones occur
    eng = GmpeEngine(cfg, device=0)
    bargs = types.SimpleNamespace(gamma=0.99, gae_lambda=0.95, use_gae=True, use_proper_time_limits=False, use_valuenorm=False, use_popart=False)
    buf = DeviceRolloutBuffer(eng, T, use_centralized_V=False, policy_fields="all", learner_fields="all", args=bargs, recurrent_N=1, hidden_size=64)
    buf.warmup()
    g = torch.Generator(device=DEV)
    g.manual_seed(17)
    for t in range(T):
        logits = torch.randn((N * A, int(cfg.n_actions)), generator=g, device=DEV)
        vals = torch.randn((N * A, 1), generator=g, device=DEV)
        rnn = torch.rand((N * A, 1, 64), generator=g, device=DEV) * 2 - 1
        buf.act_step(logits, vals, rnn_states=rnn, rnn_states_critic=rnn)
    buf.compute_returns(torch.randn((N, A, 1), generator=g, device=DEV))
    return cfg, eng, buf


def _train_nets(cfg, eng):
    F = int(cfg.node_feats)
    key = G.ACTOR if F == 7 else G.ROTATE
    assert G.CONFIGS[key]["F"] == F and int(cfg.n_actions) == K
    actor = _Net(key, eng.D, "act").to(DEV)
    critic = _Net(key, eng.D, "v_out", seed=12).to(DEV)        # the shipped critic's GNNBase is an F = 7 one: the critic here takes the actor's, with its own chain behind
    adam = lambda net: torch.optim.Adam(net.parameters(), lr=LR, eps=EPS)
    return actor, critic, adam(actor), adam(critic)


def _train_args(recurrent):
    a = update_args(max_grad_norm=0.5)
    a.ppo_epoch, a.num_mini_batch, a.data_chunk_length = 2, 2, 4
    a.use_recurrent_policy, a.use_naive_recurrent_policy = recurrent, False
    return a


def _perms(recurrent, seed=23):
    n = T * N * A // (4 if recurrent else 1)
    g = torch.Generator().manual_seed(seed)
    return [torch.randperm(n, generator=g).to(DEV) for _ in range(2)]


@pytest.mark.parametrize("recurrent", [False, True], ids=["feed-forward", "recurrent"])
def test_train_is_the_hand_written_loop_bit_for_bit(recurrent):
    cfg, eng, buf = _buffer()
    args, perms = _train_args(recurrent), _perms(recurrent)
    # train
    actor, critic, aopt, copt = _train_nets(cfg, eng)
    start = everything(actor, critic, aopt, copt)
    info = policy.train(actor, critic, aopt, copt, buf, args, perms=perms)
    got = everything(actor, critic, aopt, copt)
    # the loop of graph_mappo.py:294-359 written out
    actor, critic, aopt, copt = _train_nets(cfg, eng)
    adv = buf.normalized_advantages(None)
    sums, rows = None, []
    for e in range(2):
        gen = buf.recurrent_generator(adv, 2, 4, perm=perms[e]) if recurrent else buf.feed_forward_generator(adv, 2, perm=perms[e])
        for sample in gen:
            rows.append(int(sample[1].shape[0]))
            u = by_hand(actor, critic, aopt, copt, sample, args)
            terms = (u.value_loss, u.policy_loss, u.dist_entropy, u.actor_grad_norm, u.critic_grad_norm, u.imp_weights.mean())
            sums = terms if sums is None else tuple(a + b for a, b in zip(sums, terms))
    want_info = {k: v / 4 for k, v in zip(policy.TRAIN_INFO, sums)}
    want = everything(actor, critic, aopt, copt)
    torch.cuda.synchronize()
    assert rows == [T * N * A // 2] * 4
    assert list(info) == ["value_loss", "policy_loss", "dist_entropy", "actor_grad_norm", "critic_grad_norm", "ratio"]
    for k, v in info.items():
        assert v.dim() == 0 and v.dtype == torch.float32 and v.device.type == "cuda" and bool(torch.isfinite(v)) and same(v, want_info[k]), k
    equal_dicts(got, want)
    assert all(float(st["step"]) == 4 for opt in (aopt, copt) for st in opt.state.values())
    assert sum(not same(start[k], got[k]) for k in start if k.startswith(("actor.", "critic."))) > 40
    with pytest.raises(ValueError, match="one permutation per epoch"):
        policy.train(actor, critic, aopt, copt, buf, args, perms=perms[:1])
    eng.check_errors()
    eng.close()


def test_train_waits_for_nothing():
    """torch's sync debug mode raises at every call that waits for the device; a deliberate .item() shows that this build honours it. The permutations are
    drawn on the device: one given as a tensor is range-checked by the generator, which reads it back."""
    cfg, eng, buf = _buffer()
    args = _train_args(True)
    actor, critic, aopt, copt = _train_nets(cfg, eng)
    policy.train(actor, critic, aopt, copt, buf, args, perms=["device"] * 2)           # warm: every kernel loaded, every state created
    x = torch.ones((), device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            x.item()
        info = policy.train(actor, critic, aopt, copt, buf, args, perms=["device"] * 2)
        info2 = policy.train(actor, critic, aopt, copt, buf, args)                       # the reference's CPU randperm, uploaded from pinned memory
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(bool(torch.isfinite(v)) for v in list(info.values()) + list(info2.values()))
    assert all(float(st["step"]) == 12 for opt in (aopt, copt) for st in opt.state.values())
    eng.check_errors()
    eng.close()
