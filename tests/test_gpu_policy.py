"""gmpe.policy — the reference's actor and critic composed from the device layers — at the shape of the chain test of tests/test_gpu_gnn.py (6 steps x 5 rows,
E = 7, obs_dim 6), on modules that carry the reference's attribute names: the chain of that test plus `act` (the shipped head) or `v_out`. The logits and the
values are held to the accuracy rule against the same chain in float64 torch on the CPU (err_ref from its float32 run); the composition itself is compared
bit for bit with the layer calls written out by hand, since it adds no arithmetic of its own."""
import copy
import types

import numpy as np
import pytest
import torch

import gmpe
import gnn_lib as G
import head_lib as HL
from gmpe import policy
from test_gpu_gnn import _Chain

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L, NB, E, OBS = 6, 5, 7, 6
ROWS, K, A = L * NB, 25, 5


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).reshape(-1).view(np.uint32)


def same(a, b):
    a, b = (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in (a, b))
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


class _Net(_Chain):
    """GNNBase -> MLPBase(cat(obs, nbd)) -> RNNLayer -> the head, with the reference's attribute names. head: 'act', 'v_out' (nn.Linear) or 'popart'"""

    def __init__(self, key, obs_dim, head, use_cent_obs=True, seed=11):
        torch.manual_seed(seed)
        super().__init__(G.CONFIGS[key], obs_dim)
        self.gnn_base.load_state_dict(G.build(G.CONFIGS[key]).state_dict())
        self.args = types.SimpleNamespace(use_cent_obs=use_cent_obs)
        if head == "act":
            self.act = HL.act_layer(K, "actor")
        elif head == "v_out":
            g = HL.golden()
            self.v_out = torch.nn.Linear(64, 1)
            with torch.no_grad():
                self.v_out.weight.copy_(torch.from_numpy(g["critic.v_out.weight"]))
                self.v_out.bias.copy_(torch.from_numpy(g["critic.v_out.bias"]))

    def head_linear(self):
        return self.act.action_out.linear if hasattr(self, "act") else self.v_out


def data(key, seed=0):
    x, adj, ids, _, _ = G.inputs(ROWS, E, key)
    rng = torch.Generator().manual_seed(100 + seed)
    obs, hxs = torch.randn(ROWS, OBS, generator=rng), torch.rand(NB, 1, 64, generator=rng) * 2 - 1
    masks = (torch.rand(ROWS, 1, generator=rng) > 0.2).float()
    return obs, x, adj, ids, hxs, masks


def cpu_head(net, obs, x, adj, ids, hxs, masks, dt):
    """the head's output of the same chain in torch on the CPU in dtype dt -> float64 array"""
    ref = copy.deepcopy(net).cpu().to(dt)
    with torch.no_grad():
        f, _ = ref.torch_forward(obs.to(dt), x, adj, ids, hxs.to(dt), masks.to(dt), L)
        return ref.head_linear()(f).double().numpy()


def accurate(got, net, inputs, what):
    t64, r32 = cpu_head(net, *inputs, torch.float64), cpu_head(net, *inputs, torch.float32)
    e_ref, e_dev = HL.err(r32, t64), HL.err(got, t64)
    print("%s err_ref %.3g err_dev %.3g bound %.3g" % (what, e_ref, e_dev, HL.bound(e_ref)))
    assert e_ref <= HL.CAP and e_dev <= HL.bound(e_ref), (what, e_dev, e_ref)


def to_dev(ts):
    return [t.to(DEV) for t in ts]


def test_actor_forward_is_the_chain_and_the_fused_head():
    inputs = data(G.ACTOR)
    net = _Net(G.ACTOR, OBS, "act").to(DEV)
    obs, x, adj, ids, hxs, masks = to_dev(inputs)
    av = torch.from_numpy((np.random.RandomState(3).rand(ROWS, K) > 0.3).astype(np.float32)).to(DEV)
    av[:, K // 2] = 1.0
    logits = torch.empty((ROWS, K), device=DEV)
    kw = dict(seed=21, env_id_base=4, num_agents=A, draw=9)
    actions, logp, h = policy.actor_forward(net, obs, x, adj, ids, hxs, masks, av, out={"logits": logits}, **kw)
    full = policy.actor_forward(net, obs, x, adj, ids, hxs, masks, av, **kw)
    mode = policy.actor_forward(net, obs, x, adj, ids, hxs, masks, av, True, **kw)
    torch.cuda.synchronize()
    accurate(logits.cpu().numpy(), net, inputs, "actor_forward logits")
    with torch.no_grad():
        nbd = gmpe.gnn_base(x, adj, ids, net.gnn_base)
        f, ho = gmpe.rnn_layer(gmpe.mlp_base((obs, nbd), net.base), hxs, masks, net.rnn)
        assert same(logits, gmpe.action_logits(f, net.act))
    idx, a64, lp = gmpe.sample_actions(logits, av, **kw)
    assert actions.dtype == torch.int32 and torch.equal(actions, idx) and same(logp, lp) and same(h, ho) and not h.requires_grad
    assert full[0].dtype == torch.int64 and torch.equal(full[0], a64) and same(full[1], lp) and same(full[2], ho)
    midx, _, mlp = gmpe.sample_actions(logits, av, deterministic=True, **kw)
    assert torch.equal(mode[0].view(-1), midx.long()) and same(mode[1], mlp) and not torch.equal(mode[0], full[0])
    # an actor without an RNN: the features go straight to the head, the states come back as they were
    bare = copy.deepcopy(net)
    del bare.rnn
    out = policy.actor_forward(bare, obs, x, adj, ids, hxs, masks, av, **kw)
    with torch.no_grad():
        want = gmpe.act_head(gmpe.mlp_base((obs, nbd), net.base), net.act, av, **kw)
    assert torch.equal(out[0], want[1]) and same(out[1], want[2]) and out[2] is hxs


@pytest.mark.parametrize("cent", [True, False])
def test_critic_forward_meets_the_accuracy_rule(cent):
    obs, x, adj, ids, hxs, masks = inputs = data(G.CRITIC, seed=1)
    net = _Net(G.CRITIC, OBS if cent else 0, "v_out", use_cent_obs=cent).to(DEV)
    d = to_dev(inputs)
    values, h = policy.critic_forward(net, *d)
    assert tuple(values.shape) == (ROWS, 1) and tuple(h.shape) == (NB, 1, 64) and values.requires_grad
    values.sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    torch.cuda.synchronize()
    ref_inputs = inputs if cent else (obs[:, :0],) + tuple(inputs[1:])
    accurate(values.detach().cpu().numpy(), net, ref_inputs, "critic_forward values, use_cent_obs=%s" % cent)
    nbd = gmpe.gnn_base(d[1], d[2], d[3], net.gnn_base)
    f, ho = gmpe.rnn_layer(gmpe.mlp_base((d[0], nbd) if cent else nbd, net.base), d[4], d[5], net.rnn)
    assert same(values, torch.nn.functional.linear(f, net.v_out.weight, net.v_out.bias)) and same(h, ho)
    # several ids per row (critic_graph_aggr == "node") is gnn_base's refusal, let through
    with pytest.raises(NotImplementedError, match="ids per row"):
        policy.critic_forward(net, d[0], d[1], d[2], d[3].view(-1, 1).repeat(1, 3), d[4], d[5])


def sample_of(seed=2):
    obs, x, adj, ids, hxs, masks = data(G.ACTOR, seed=seed)
    rng = np.random.RandomState(40 + seed)
    f32 = np.float32
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    share_obs, hxs_c = t(rng.randn(ROWS, OBS).astype(f32)), t(rng.uniform(-1, 1, (NB, 1, 64)).astype(f32))
    av = (rng.rand(ROWS, K) > 0.3).astype(f32)
    av[:, K // 2] = 1.0
    actions = np.array([rng.choice(np.flatnonzero(r)) for r in av], np.float32).reshape(ROWS, 1)
    cols = [t(actions), t(rng.randn(ROWS, 1).astype(f32)), t(rng.randn(ROWS, 1).astype(f32)), masks, t((rng.rand(ROWS, 1) > 0.1).astype(f32)),
            t((-rng.rand(ROWS, 1) * 3).astype(f32)), t(rng.randn(ROWS, 1).astype(f32)), t(av)]
    return tuple(to_dev([share_obs, obs, x, adj, ids, ids.clone(), hxs, hxs_c] + cols))


def loss_args(**over):
    kw = dict(clip_param=0.2, huber_delta=10.0, entropy_coef=0.01, use_policy_active_masks=True, use_value_active_masks=True, use_clipped_value_loss=True,
              use_huber_loss=True, use_valuenorm=False, use_popart=False)
    kw.update(over)
    return types.SimpleNamespace(**kw)


def by_hand(actor, critic, s, args):
    nbd = gmpe.gnn_base(s[2], s[3], s[4], actor.gnn_base)
    f, _ = gmpe.rnn_layer(gmpe.mlp_base((s[1], nbd), actor.base), s[6], s[11], actor.rnn)
    logits = gmpe.action_logits(f, actor.act)
    nbd_c = gmpe.gnn_base(s[2], s[3], s[5], critic.gnn_base)
    fc, _ = gmpe.rnn_layer(gmpe.mlp_base((s[0], nbd_c), critic.base), s[7], s[11], critic.rnn)
    if args.use_popart:
        return gmpe.ppo_losses_popart(logits, fc, s, args, critic.v_out)
    return gmpe.ppo_losses(logits, torch.nn.functional.linear(fc, critic.v_out.weight, critic.v_out.bias), s, args)


def finish(res, actor, critic, v_params):
    (res.actor_loss * 1).backward()
    (res.value_loss * 1).backward()
    torch.cuda.synchronize()
    grads = {"actor." + k: p.grad for k, p in actor.named_parameters()}
    grads.update({"critic." + k: p.grad for k, p in critic.named_parameters()})
    grads.update({"v_out.%d" % i: p.grad for i, p in enumerate(v_params)})
    scalars = {k: getattr(res, k).detach().cpu().numpy() for k in res._fields}
    return scalars, grads


@pytest.mark.parametrize("popart", [False, True], ids=["plain", "popart"])
def test_minibatch_losses_is_the_hand_written_sequence_bit_for_bit(popart):
    s = sample_of()
    args = loss_args(use_popart=popart)
    runs = []
    for fn in (lambda a, c: policy.minibatch_losses(a, c, s, args), lambda a, c: by_hand(a, c, s, args)):
        actor = _Net(G.ACTOR, OBS, "act").to(DEV)
        critic = _Net(G.CRITIC, OBS, "popart" if popart else "v_out", seed=12).to(DEV)
        if popart:
            critic.v_out = HL.PopArt(DEV)
        v_params = [critic.v_out.weight, critic.v_out.bias] if popart else []       # install="replace" swaps the objects: the ones of the call get the gradients
        runs.append(finish(fn(actor, critic), actor, critic, v_params))
    (sa, ga), (sb, gb) = runs
    assert sorted(sa) == sorted(sb) and sorted(ga) == sorted(gb) and ("values" in sa) == popart
    for k in sa:
        assert same(sa[k], sb[k]), k
    for k in ga:
        assert ga[k] is not None and gb[k] is not None, "no gradient reached " + k
        assert same(ga[k], gb[k]), k
        # a key bias shifts every score of a target alike, which the softmax does not see: its gradient is rounding noise around zero, or zero
        assert bool(torch.isfinite(ga[k]).all()) and (float(ga[k].abs().max()) > 0 or "lin_key.bias" in k), k
    assert np.isfinite(sa["actor_loss"]).all() and np.isfinite(sa["value_loss"]).all() and sa["imp_weights"].shape == (ROWS, 1)


def equal(a, b):
    """two summaries (nested dicts of numbers and arrays), NaN equal to NaN"""
    if isinstance(a, dict) or isinstance(b, dict):
        return isinstance(a, dict) and isinstance(b, dict) and sorted(a) == sorted(b) and all(equal(a[k], b[k]) for k in a)
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


def test_evaluator_act_drives_a_batched_evaluator_like_the_loop_written_out():
    from gmpe import evaluate as EV
    from gmpe.engine import GmpeEngine
    N, T = 4, 8
    cfg = gmpe.make_config(num_envs=N, num_agents=3, episode_length=T, seed=3)
    A = cfg.num_agents
    summaries = []
    for adj_compact in (False, True):                   # either adjacency form the engine hands out
        eng = GmpeEngine(cfg, 0, adj_compact=adj_compact)
        F, D, rows = int(cfg.node_feats), eng.D, N * A
        key = G.ACTOR if F == 7 else G.ROTATE
        assert G.CONFIGS[key]["F"] == F and int(cfg.n_actions) == K
        net = _Net(key, D, "act").to(DEV)
        state = eng.get_state()
        rnn = torch.zeros((N, A, 1, 64), device=DEV)
        ev = EV.BatchedEvaluator(eng, rnn_states=rnn)
        got = EV.evaluate(eng, policy.evaluator_act(net, ev, deterministic=False, seed=5, draw0=3), evaluator=ev)
        got_rnn = rnn.clone()
        # ... and the same loop with the layer calls written out
        eng.set_state(state)
        rnn2 = torch.zeros((N, A, 1, 64), device=DEV)
        ev2 = EV.BatchedEvaluator(eng, rnn_states=rnn2)
        o = ev2.reset()
        for t in range(T):
            with torch.no_grad():
                nbd = gmpe.gnn_base(o.node_obs.reshape(rows, -1, F), o.adj.reshape(-1, eng.E, eng.E), o.agent_id.reshape(rows), net.gnn_base)
                f, h = gmpe.rnn_layer(gmpe.mlp_base((o.obs.reshape(rows, D), nbd), net.base), rnn2.view(rows, 1, 64), ev2.masks.view(rows, 1), net.rnn)
                idx, _, _ = gmpe.sample_actions(gmpe.action_logits(f, net.act), ev2.available_actions.view(rows, K), seed=5,
                                                env_id_base=int(cfg.env_id_base), num_agents=A, draw=3 + t)
                rnn2.copy_(h.view(N, A, 1, 64))
            o = eng.step(idx.view(N, A))
            ev2.record()
        want = ev2.summary()
        assert got["episodes"] == N and equal(got, want), (got, want)
        assert same(got_rnn, rnn2)
        summaries.append(got)
    assert equal(summaries[0], summaries[1])            # the compact adjacency gives the materialised form's bits, so the same episodes
    with pytest.raises(ValueError, match="rnn_states"):
        policy.evaluator_act(net, EV.BatchedEvaluator(eng))
