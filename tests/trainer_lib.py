"""What the tests of the composed learner (gmpe.policy.ppo_update / train / actor_forward / critic_forward) share: the fixtures of
tests/golden/make_trainer_fixture.py — the reference's own GR_MAPPO.ppo_update and GR_MAPPO.train on its own GR_Actor / GR_Critic, run in float64 (the
truth) and in float32 (err_ref) —, mirror modules that carry the reference's attribute names and load the fixture's state_dict with strict=True, the
same trainer written out in plain torch (torch's own clip_grad_norm_ and Adam, in the reference's order), and the metric.

The mirrors are tests/test_gpu_policy.py's _Net plus the reference's MLPLayer.fc_h (mlp.py:30-35: the template fc2 is cloned from; it never runs, so it
never receives a gradient and Adam never gives it state) and, with --use_popart, a PopArt module (popart.py). The plain-torch trainer runs them on the
CPU in float64, where it must reproduce the truth (tests/test_trainer_host.py); gmpe.policy runs them on the device.

The metric is optim_lib's: err(a, t) = max|a - t| / max|t| on each network's tensors concatenated into one array per kind (clipped grad, exp_avg,
exp_avg_sq, param) — per tensor the lin_key.bias gradients are pure cancellation noise around a truth of 1e-17 — and on every scalar;
err_dev <= 4 * err_ref + 2^-23 with err_ref <= 1e-5. The step is judged through `param`, not through param - initial: Adam's step is scale-free per
element, so float32 noise in a gradient near eps is amplified in the difference (the reference's own float32 run is 1e-4 off there)."""
import functools
import json
import os
import types

import numpy as np
import torch
import torch.nn.functional as F

import gnn_lib as G
from optim_lib import CAP, bound, err  # noqa: F401  (the rule, shared)
from test_gpu_policy import K, L, NB, OBS, ROWS, E, _Net  # noqa: F401  (the shapes, shared)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LR, EPS = 5e-4, 1e-5
KINDS = ("grad", "exp_avg", "exp_avg_sq", "param")
SCALARS = ("value_loss", "critic_grad_norm", "policy_loss", "dist_entropy", "actor_grad_norm", "ratio_mean")
TRAIN_INFO = ("value_loss", "policy_loss", "dist_entropy", "actor_grad_norm", "critic_grad_norm", "ratio")
SAMPLE = ("share_obs", "obs", "node_obs", "adj", "agent_id", "share_agent_id", "rnn_states", "rnn_states_critic", "actions", "value_preds", "returns",
          "masks", "active_masks", "old_action_log_probs", "adv_targ", "available_actions")
UPDATES = 3
# case -> (args over BASE_ARGS, update_actor, the networks whose arrays are stored). The clip bites in every case that clips.
BASE_ARGS = dict(clip_param=0.2, huber_delta=10.0, entropy_coef=0.01, use_policy_active_masks=True, use_value_active_masks=True,
                 use_clipped_value_loss=True, use_huber_loss=True, use_valuenorm=False, use_popart=False, use_max_grad_norm=True, max_grad_norm=0.01,
                 value_loss_coef=0.5, use_recurrent_policy=True, use_naive_recurrent_policy=False, ppo_epoch=2, num_mini_batch=2, data_chunk_length=4)
CASES = {"plain": ({}, True, ("actor", "critic")), "valuenorm": (dict(use_valuenorm=True), True, ("critic",)),
         "popart": (dict(use_popart=True), True, ("critic",)), "no-actor": ({}, False, ("critic",)),
         "no-clip": (dict(use_max_grad_norm=False), True, ("actor",))}
TRAIN_CASES = {"train-recurrent": dict(max_grad_norm=0.5), "train-feed-forward": dict(max_grad_norm=0.5, use_recurrent_policy=False)}
MAX_FILE = 767956                                       # the largest fixture tests/golden held before these (gru_layer_ones.npz)


def case_args(case):
    kw = dict(BASE_ARGS)
    kw.update(CASES[case][0] if case in CASES else TRAIN_CASES[case])
    return types.SimpleNamespace(**kw)


# ---------------------------------------------------------------------------------------------- the mirrors
class PopArt(torch.nn.Module):
    """the reference's PopArt(64, 1) (popart.py), attribute for attribute: six Parameters, update() in its order with its aliased old_mean"""

    def __init__(self):
        super().__init__()
        P = torch.nn.Parameter
        self.beta, self.epsilon, self.norm_axes, self.output_shape = 0.99999, 1e-5, 1, 1
        self.weight, self.bias = P(torch.zeros(1, 64)), P(torch.zeros(1))
        self.stddev, self.mean, self.mean_sq = (P(v, requires_grad=False) for v in (torch.ones(1), torch.zeros(1), torch.zeros(1)))
        self.debiasing_term = P(torch.tensor(0.0), requires_grad=False)

    @torch.no_grad()
    def update(self, x):
        old_mean, old_stddev = self.mean, self.stddev                   # popart.py:68: old_mean is the tensor the next line writes
        self.mean.mul_(self.beta).add_(x.mean(0) * (1.0 - self.beta))
        self.mean_sq.mul_(self.beta).add_((x ** 2).mean(0) * (1.0 - self.beta))
        self.debiasing_term.mul_(self.beta).add_(1.0 * (1.0 - self.beta))
        self.stddev = torch.nn.Parameter((self.mean_sq - self.mean ** 2).sqrt().clamp(min=1e-4))
        self.weight = torch.nn.Parameter(self.weight * old_stddev / self.stddev)
        self.bias = torch.nn.Parameter((old_stddev * self.bias + old_mean - self.mean) / self.stddev)

    def normalize(self, x):
        mean = self.mean / self.debiasing_term.clamp(min=self.epsilon)
        var = (self.mean_sq / self.debiasing_term.clamp(min=self.epsilon) - mean ** 2).clamp(min=1e-2)
        return (x - mean[None]) / torch.sqrt(var)[None]


class ValueNorm(object):
    """the three tensors of the reference's ValueNorm(1) (valuenorm.py), fresh, with its update and normalize"""

    def __init__(self, device="cpu", dtype=torch.float32):
        self.beta, self.epsilon, self.norm_axes, self.per_element_update = 0.99999, 1e-5, 1, False
        self.running_mean, self.running_mean_sq = torch.zeros(1, device=device, dtype=dtype), torch.zeros(1, device=device, dtype=dtype)
        self.debiasing_term = torch.zeros((), device=device, dtype=dtype)

    @torch.no_grad()
    def update(self, x):
        self.running_mean.mul_(self.beta).add_(x.mean(0) * (1.0 - self.beta))
        self.running_mean_sq.mul_(self.beta).add_((x ** 2).mean(0) * (1.0 - self.beta))
        self.debiasing_term.mul_(self.beta).add_(1.0 * (1.0 - self.beta))

    def normalize(self, x):
        mean = self.running_mean / self.debiasing_term.clamp(min=self.epsilon)
        var = (self.running_mean_sq / self.debiasing_term.clamp(min=self.epsilon) - mean ** 2).clamp(min=1e-2)
        return (x - mean[None]) / torch.sqrt(var)[None]


class Net(_Net):
    """_Net with the reference's fc_h and its two recurrence flags; head: 'act', 'v_out' or 'popart'. Without use_recurrent_policy the reference
    builds no RNNLayer (graph_actor_critic.py:88-90), so there is none. The weights come from load_state_dict."""

    def __init__(self, head, recurrent=True):
        key = G.ACTOR if head == "act" else G.CRITIC
        super().__init__(key, OBS, "v_out" if head == "popart" else head)
        nn = torch.nn
        self.base.mlp.fc_h = nn.Sequential(nn.Linear(64, 64), nn.ReLU(), nn.LayerNorm(64))
        self._use_recurrent_policy, self._use_naive_recurrent_policy = bool(recurrent), False
        if not recurrent:
            del self.rnn
        if head == "popart":
            self.v_out = PopArt()

    def features(self, own, x, adj, ids, hxs, masks):
        if self._use_recurrent_policy:
            return self.torch_forward(own, x, adj, ids.reshape(-1), hxs, masks, own.shape[0] // hxs.shape[0])
        nbd = G.forward(self.gnn_base, x.to(own.dtype), adj.to(own.dtype), ids.reshape(-1))
        return self.base.mlp.fc2[0](self.base.mlp.fc1(self.base.feature_norm(torch.cat([own, nbd], 1)))), hxs


def nets(fx, popart=False, device="cpu", dtype=torch.float32, recurrent=True):
    """(actor, critic, actor_optimizer, critic_optimizer, born) from the fixture's initial state_dicts, loaded strictly; born: id(parameter) -> the
    name it had when its optimiser was built"""
    actor, critic = Net("act", recurrent), Net("popart" if popart else "v_out", recurrent)
    actor.load_state_dict({k: torch.from_numpy(v) for k, v in fx["init"]["actor"].items()}, strict=True)
    critic.load_state_dict({k: torch.from_numpy(v) for k, v in fx["init"]["critic_popart" if popart else "critic"].items()}, strict=True)
    actor, critic = actor.to(device=device, dtype=dtype), critic.to(device=device, dtype=dtype)
    adam = lambda net: torch.optim.Adam(net.parameters(), lr=LR, eps=EPS, weight_decay=0)
    born = {id(p): "%s.%s" % (tag, k) for tag, net in (("actor", actor), ("critic", critic)) for k, p in net.named_parameters()}
    return actor, critic, adam(actor), adam(critic), born


# ---------------------------------------------------------------------------------------------- the trainer in plain torch
def torch_losses(actor, critic, s, args, vn):
    """evaluate_actions and the loss arithmetic of GR_MAPPO.ppo_update (graph_mappo.py:147-200, 239-242) -> (value_loss, policy_loss, dist_entropy,
    imp_weights); the flags are the cases' (both active masks, the clipped value loss, the Huber loss)"""
    assert args.use_policy_active_masks and args.use_value_active_masks and args.use_clipped_value_loss and args.use_huber_loss
    share_obs, obs, x, adj, ids, sids, h, hc, actions, vpred, ret, masks, active, old_lp, adv, avail = s
    f, _ = actor.features(obs, x, adj, ids, h, masks)
    logits = actor.act.action_out.linear(f)
    logits = logits.masked_fill(avail == 0, torch.finfo(logits.dtype).min)                     # distributions.py:89
    dist = torch.distributions.Categorical(logits=logits)
    lp = dist.log_prob(actions.squeeze(-1).long()).unsqueeze(-1)
    dist_entropy = (dist.entropy() * active.squeeze(-1)).sum() / active.sum()
    fc, _ = critic.features(share_obs, x, adj, sids, hc, masks)
    values = F.linear(fc, critic.v_out.weight, critic.v_out.bias)
    imp = torch.exp(lp - old_lp)
    surr = torch.min(imp * adv, torch.clamp(imp, 1.0 - args.clip_param, 1.0 + args.clip_param) * adv)
    policy_loss = (-surr.sum(-1, keepdim=True) * active).sum() / active.sum()
    clipped = vpred + (values - vpred).clamp(-args.clip_param, args.clip_param)
    norm = critic.v_out if args.use_popart else (vn if args.use_valuenorm else None)
    if norm is not None:
        norm.update(ret)
        ret = norm.normalize(ret)
    d = args.huber_delta
    huber = lambda e: (e.abs() <= d).to(e.dtype) * e ** 2 / 2 + (e > d).to(e.dtype) * d * (e.abs() - d / 2)      # util.py:24-27, its one-sided b
    value_loss = (torch.max(huber(ret - values), huber(ret - clipped)) * active).sum() / active.sum()
    return value_loss, policy_loss, dist_entropy, imp


def torch_ppo_update(actor, critic, aopt, copt, s, args, vn=None, update_actor=True):
    """GR_MAPPO.ppo_update (graph_mappo.py:147-278) with torch's own clip and Adam -> the six SCALARS and imp_weights"""
    value_loss, policy_loss, dist_entropy, imp = torch_losses(actor, critic, s, args, vn)
    clip = torch.nn.utils.clip_grad_norm_ if args.use_max_grad_norm else \
        (lambda ps, _: torch.sqrt(sum((p.grad.norm() ** 2 for p in ps if p.grad is not None), torch.zeros((), dtype=imp.dtype))))
    aopt.zero_grad()
    if update_actor:
        (policy_loss - dist_entropy * args.entropy_coef).backward()
    an = clip(list(actor.parameters()), args.max_grad_norm)
    if update_actor:
        aopt.step()
    copt.zero_grad()
    (value_loss * args.value_loss_coef).backward()
    cn = clip(list(critic.parameters()), args.max_grad_norm)
    copt.step()
    return (value_loss.detach(), cn, policy_loss.detach(), dist_entropy.detach(), an, imp.detach().mean()), imp.detach()


def torch_train(actor, critic, aopt, copt, buffer, args, update=torch_ppo_update):
    """GR_MAPPO.train (graph_mappo.py:294-359) over a buffer with the DeviceRolloutBuffer's methods -> train_info"""
    adv = buffer.normalized_advantages(None)
    info = dict.fromkeys(TRAIN_INFO, 0.0)
    for _ in range(args.ppo_epoch):
        gen = buffer.recurrent_generator(adv, args.num_mini_batch, args.data_chunk_length) if args.use_recurrent_policy else \
            buffer.feed_forward_generator(adv, args.num_mini_batch)
        for s in gen:
            (vl, cn, pl, ent, an, _), imp = update(actor, critic, aopt, copt, s, args)
            for k, v in zip(TRAIN_INFO, (vl, pl, ent, an, cn, imp.mean())):
                info[k] = info[k] + v
    return {k: v / (args.ppo_epoch * args.num_mini_batch) for k, v in info.items()}


# ---------------------------------------------------------------------------------------------- what is compared
def entries(net, opt, born):
    """[(name, parameter)]: the network's named_parameters(), then what its optimiser holds and the network no longer does — the v_out objects a
    PopArt update replaced — as 'old:<the name it had>'"""
    tag = born[id(next(iter(net.parameters())))].split(".")[0]
    out = [("%s.%s" % (tag, k), p) for k, p in net.named_parameters()]
    have = set(id(p) for _, p in out)
    return out + [("old:" + born[id(p)], p) for g in opt.param_groups for p in g["params"] if id(p) not in have]


def collect(net, opt, born):
    """{name: {'param', 'grad' or None, 'exp_avg' or None, 'exp_avg_sq' or None, 'step'}} as float64 arrays"""
    f = lambda t: t.detach().double().cpu().numpy().reshape(-1).copy()
    out = {}
    for name, p in entries(net, opt, born):
        st = opt.state.get(p, {})
        out[name] = dict(param=f(p), grad=None if p.grad is None else f(p.grad), exp_avg=f(st["exp_avg"]) if st else None,
                         exp_avg_sq=f(st["exp_avg_sq"]) if st else None, step=int(float(st["step"])) if st else 0)
    return out


def arrays_of(got, meta):
    """the four concatenations in the fixture's order; where state and gradients lie must be where the reference has them, to the name"""
    assert sorted(got) == sorted(meta["names"]), sorted(set(got) ^ set(meta["names"]))
    for name, size, has_grad, step in zip(meta["names"], meta["sizes"], meta["has_grad"], meta["steps"]):
        g = got[name]
        assert g["param"].size == size, name
        assert (g["grad"] is not None) == bool(has_grad), "%s: gradient %s" % (name, "missing" if has_grad else "unexpected")
        assert g["step"] == step and (g["exp_avg"] is not None) == (step > 0), "%s: %d steps, the reference %d" % (name, g["step"], step)
    cat = lambda kind: np.concatenate([got[n][kind] for n in meta["names"] if got[n][kind] is not None] or [np.zeros(0)])
    return {kind: cat(kind) for kind in KINDS}


# ---------------------------------------------------------------------------------------------- the fixtures
def _npz(name):
    with np.load(os.path.join(GOLDEN, name)) as d:
        return {k: d[k] for k in d.files}


def files():
    return sorted(f for f in os.listdir(GOLDEN) if f.startswith("trainer_") and f.endswith(".npz"))


@functools.lru_cache(maxsize=None)
def inputs():
    """the initial state_dicts (the reference's names), the three samples of the ppo_update cases and the forward record"""
    d = _npz("trainer_inputs.npz")
    init = {}
    for k, v in d.items():
        if k.startswith("init:"):
            _, net, name = k.split(":")
            init.setdefault(net, {})[name] = v
    samples = [tuple(d["sample%d:%s" % (i, k)] for k in SAMPLE) for i in range(UPDATES)]
    forward = {k.split(":", 1)[1]: v for k, v in d.items() if k.startswith("forward:")}
    return dict(init=init, samples=samples, forward=forward)


@functools.lru_cache(maxsize=None)
def load(case):
    """one case: 'meta' (per network the names, sizes, has_grad, steps and the err_ref per kind), the scalars and imp_weights with their err_ref,
    the float64 arrays per stored network, and for a train case the recorded generator calls"""
    tag = case.replace("-", "_")
    d = _npz("trainer_%s.npz" % tag)
    fx = dict(inputs(), case=case, args=json.loads(str(d["args"])), raw=d, meta={}, truth={}, err_ref={})
    own = [k for k in d if k.startswith("init:")]       # a train case whose seed is not the ppo_update cases' brings its own initial state
    if own:
        fx["init"] = {}
        for k in own:
            fx["init"].setdefault(k.split(":")[1], {})[k.split(":")[2]] = d[k]
    for net in json.loads(str(d["stored"])):
        fx["meta"][net] = {k: d["%s:%s" % (net, k)] for k in ("names", "sizes", "has_grad", "steps")}
        fx["meta"][net]["names"] = [str(n) for n in fx["meta"][net]["names"]]
        fx["truth"][net], fx["err_ref"][net] = {}, {}
        for half in ("gp", "mv"):
            a = _npz("trainer_%s_%s_%s.npz" % (tag, net, half))
            fx["truth"][net].update(a)
        for kind in KINDS:
            fx["err_ref"][net][kind] = float(d["%s:err_ref:%s" % (net, kind)])
    return fx


def sample_on(s, device, dtype):
    """a recorded 16-tuple as tensors: the floats in `dtype`, the ids as they were recorded"""
    out = []
    for a in s:
        t = torch.from_numpy(np.ascontiguousarray(a)).to(device)
        out.append(t.to(dtype) if t.is_floating_point() else t)
    return tuple(out)


class ReplayBuffer(object):
    """What GR_MAPPO.train asked of the reference's GraphReplayBuffer, replayed: normalized_advantages returns the recorded array, and each generator
    call must be the recorded method with the recorded arguments, in the recorded order; it yields that call's recorded samples."""

    def __init__(self, fx, device, dtype):
        d = fx["raw"]
        self.calls = json.loads(str(d["calls"]))                            # [[method, num_mini_batch, data_chunk_length or None, samples]]
        self.adv = torch.from_numpy(d["advantages"]).to(device=device, dtype=dtype)
        self.samples = [sample_on(tuple(d["yield%d:%s" % (i, k)] for k in SAMPLE), device, dtype) for i in range(sum(c[3] for c in self.calls))]
        self.at, self.given = 0, 0

    def normalized_advantages(self, value_normalizer=None):
        assert value_normalizer is None
        return self.adv

    def _replay(self, method, advantages, num_mini_batch, chunk, perm):
        assert self.at < len(self.calls), "more generator calls than the reference made"
        assert [method, int(num_mini_batch), chunk] == self.calls[self.at][:3], ((method, num_mini_batch, chunk), self.calls[self.at])
        assert advantages is self.adv and perm is None
        n = self.calls[self.at][3]
        self.at += 1
        for _ in range(n):
            self.given += 1
            yield self.samples[self.given - 1]

    def recurrent_generator(self, advantages, num_mini_batch, data_chunk_length, perm=None):
        return self._replay("recurrent_generator", advantages, num_mini_batch, int(data_chunk_length), perm)

    def feed_forward_generator(self, advantages, num_mini_batch, perm=None):
        return self._replay("feed_forward_generator", advantages, num_mini_batch, None, perm)

    def naive_recurrent_generator(self, advantages, num_mini_batch):
        return self._replay("naive_recurrent_generator", advantages, num_mini_batch, None, None)

    def exhausted(self):
        return self.at == len(self.calls) and self.given == len(self.samples)


# ---------------------------------------------------------------------------------------------- running a case
def run_updates(fx, update, device, dtype):
    """the case's three updates on fresh mirrors -> (scalars [3, 6] float64, imp_weights [3, rows, 1] float64, {network: collect(...)}, the mirrors).
    update(actor, critic, aopt, copt, sample, args, vn, update_actor) -> (the six SCALARS, imp_weights)"""
    case = fx["case"]
    args = types.SimpleNamespace(**fx["args"])
    actor, critic, aopt, copt, born = nets(fx, args.use_popart, device, dtype)
    vn = ValueNorm(device, dtype) if args.use_valuenorm else None
    scalars, imps = [], []
    for s in fx["samples"]:
        sc, imp = update(actor, critic, aopt, copt, sample_on(s, device, dtype), args, vn, CASES[case][1])
        scalars.append([float(v) for v in sc])
        imps.append(imp.detach().double().cpu().numpy())
    got = {"actor": collect(actor, aopt, born), "critic": collect(critic, copt, born)}
    return np.array(scalars), np.array(imps), got, (actor, critic, aopt, copt, vn)


def run_train(fx, train, device, dtype):
    """train(actor, critic, aopt, copt, buffer, args) -> train_info on fresh mirrors -> (the six TRAIN_INFO values, {network: collect(...)})"""
    args = types.SimpleNamespace(**fx["args"])
    actor, critic, aopt, copt, born = nets(fx, False, device, dtype, args.use_recurrent_policy)
    buf = ReplayBuffer(fx, device, dtype)
    info = train(actor, critic, aopt, copt, buf, args)
    assert list(info) == list(TRAIN_INFO) and buf.exhausted()
    return np.array([float(info[k]) for k in TRAIN_INFO]), {"actor": collect(actor, aopt, born), "critic": collect(critic, copt, born)}


def compare(fx, scalars, got, names, what, limit, imps=None):
    """every stored array and scalar of a case against the truth; limit(err_ref) is the bound. Prints each figure, then asserts; -> the worst
    err / bound"""
    rows = []
    for net in fx["meta"]:
        a = arrays_of(got[net], fx["meta"][net])
        for kind in KINDS:
            rows.append(("%s %s" % (net, kind), err(a[kind], fx["truth"][net][kind]), fx["err_ref"][net][kind]))
    t, e = fx["raw"]["scalars"], fx["raw"]["scalars:err_ref"]
    assert scalars.shape == t.shape
    for i in np.ndindex(*t.shape):
        label = "%s %s" % (names[i[-1]], "" if t.ndim == 1 else "update %d" % i[0])
        if t[i] == 0.0:                                 # the actor's norm without update_actor: exactly zero in the reference, so exactly zero
            assert scalars[i] == 0.0, label
        else:
            rows.append((label, err(scalars[i], t[i]), float(e[i])))
    if imps is not None:
        rows.append(("imp_weights", err(imps, fx["raw"]["imp_weights"]), float(fx["raw"]["imp_weights:err_ref"])))
    for label, e_dev, e_ref in rows:
        print("%s %-28s err_ref %.3g err %.3g bound %.3g" % (what, label, e_ref, e_dev, limit(e_ref)))
    for label, e_dev, e_ref in rows:
        assert e_ref <= CAP and e_dev <= limit(e_ref), (what, label, e_dev, e_ref)
    return max(e_dev / limit(e_ref) for _, e_dev, e_ref in rows)
