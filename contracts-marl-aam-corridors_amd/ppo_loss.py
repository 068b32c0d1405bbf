"""The loss arithmetic of GR_MAPPO.ppo_update on the device (include/gmpe.h gmpe_ppo_loss): logits and values in, two differentiable scalars out.

    for sample in dbuf.feed_forward_generator(advantages, num_mini_batch):
        logits = actor.act.action_out.linear(actor_features)          # the head's linear layer, before Categorical masks it
        res = gmpe.ppo_losses(logits, values, sample, args, value_normalizer)
        scaler.scale(res.actor_loss).backward()
        scaler.scale(res.value_loss * args.value_loss_coef).backward()

One call of gmpe_ppo_loss (four launches) evaluates the masked categorical (onpolicy/algorithms/utils/distributions.py:84-91, act.py:212-220), the
ratio / clip / surrogate block (onpolicy/algorithms/graph_mappo.py:176-197) and cal_value_loss with ValueNorm.update + normalize (:89-117,
onpolicy/utils/valuenorm.py:48-85), and leaves d actor_loss / d logits and d value_loss / d values; backward multiplies them by the incoming
scalar. There is no torch fallback: the arrays must be on a HIP device.

With --use_popart the value normaliser is the critic's output layer, so the critic hands over its features and ppo_losses_popart (gmpe_ppo_loss_popart)
evaluates that layer, updates and rescales it, and leaves the gradients of features, weight and bias:

        res = gmpe.ppo_losses_popart(logits, critic_features, sample, args, critic.v_out)
"""
import collections
import ctypes as C

import torch

from . import _lib
from .engine import _need_cuda, _ordinal, _stream_of, _workspace

PPOPopArtLosses = collections.namedtuple("PPOPopArtLosses", ["actor_loss", "value_loss", "policy_loss", "dist_entropy", "ratio_mean", "action_log_probs",
                                                             "imp_weights", "values"])
PPOLosses = collections.namedtuple("PPOLosses", ["actor_loss", "value_loss", "policy_loss", "dist_entropy", "ratio_mean", "action_log_probs",
                                                 "imp_weights"])
FIELDS = ("actions", "value_preds", "returns", "active_masks", "old_action_log_probs", "adv_targ", "available_actions")
# positions in the 16-tuple of GraphReplayBuffer's generators (graph_mappo.py:147-151)
_TUPLE = dict(actions=8, value_preds=9, returns=10, active_masks=12, old_action_log_probs=13, adv_targ=14, available_actions=15)
_DEFAULTS = dict(clip_param=0.2, huber_delta=10.0, entropy_coef=0.01, use_policy_active_masks=True, use_value_active_masks=True,
                 use_clipped_value_loss=True, use_huber_loss=True, use_valuenorm=True, use_popart=False)


def workspace_bytes(rows):
    """Device scratch (bytes) one ppo_losses call over `rows` rows needs (gmpe_ppo_loss_workspace_bytes)."""
    n = C.c_size_t()
    _lib.check(_lib.load().gmpe_ppo_loss_workspace_bytes(int(rows), C.byref(n)), "gmpe_ppo_loss_workspace_bytes")
    return int(n.value)


def _fields(sample):
    if isinstance(sample, dict):
        unknown = set(sample) - set(FIELDS)
        if unknown:
            raise ValueError("unknown fields: %s (expected %s)" % (sorted(unknown), list(FIELDS)))
        f = {k: sample.get(k) for k in FIELDS}
    elif isinstance(sample, (tuple, list)) and len(sample) == 16:
        f = {k: sample[i] for k, i in _TUPLE.items()}
    else:
        raise ValueError("sample_or_fields must be the generators' 16-tuple or a dict with %s" % (list(FIELDS),))
    missing = [k for k in FIELDS[:-1] if f[k] is None]
    if missing:
        raise ValueError("the sample holds no %s" % ", ".join(missing))
    return f


def _flags(args, popart=False):
    get = lambda k: getattr(args, k, _DEFAULTS[k])
    if popart:
        if not get("use_popart"):
            raise ValueError("args.use_popart is not set: ppo_losses_popart is the --use_popart path, ppo_losses the other")
        if getattr(args, "use_valuenorm", False):
            raise ValueError("use_popart and use_valuenorm can not be set True simultaneously")        # graph_mappo.py:61
    elif get("use_popart"):
        raise NotImplementedError("use_popart: PopArt rewrites the critic's output layer, so the critic hands over its features, not its values: "
                                  "call ppo_losses_popart(logits, critic_features, sample, args, critic.v_out); ppo_losses supports ValueNorm or no "
                                  "normaliser")
    flags = 0
    for name, bit in (("use_policy_active_masks", _lib.PPO_POLICY_ACTIVE_MASKS), ("use_value_active_masks", _lib.PPO_VALUE_ACTIVE_MASKS),
                      ("use_clipped_value_loss", _lib.PPO_CLIPPED_VALUE_LOSS), ("use_huber_loss", _lib.PPO_HUBER_LOSS),
                      ("use_valuenorm", _lib.PPO_VALUENORM)):
        if get(name) and not (popart and bit == _lib.PPO_VALUENORM):
            flags |= bit
    return flags, float(get("clip_param")), float(get("huber_delta")), float(get("entropy_coef"))


def _valuenorm_state(vn, dev):
    """The three tensors of the reference's ValueNorm(1) (valuenorm.py:34-39), updated in place by the kernel."""
    if vn is None:
        raise ValueError("args.use_valuenorm is set, so a value_normalizer (ValueNorm) is required")
    names = ("running_mean", "running_mean_sq", "debiasing_term")
    if not all(isinstance(getattr(vn, n, None), torch.Tensor) for n in names):
        raise NotImplementedError("value_normalizer must be a ValueNorm (running_mean, running_mean_sq, debiasing_term); PopArt is not supported")
    if int(getattr(vn, "norm_axes", 1)) != 1 or bool(getattr(vn, "per_element_update", False)) or vn.running_mean.numel() != 1 or \
            vn.running_mean_sq.numel() != 1 or vn.debiasing_term.numel() != 1:
        raise NotImplementedError("only ValueNorm(1) is supported: input_shape 1, norm_axes 1, per_element_update=False")
    st = [getattr(vn, n) for n in names]
    for n, t in zip(names, st):
        if t.dtype != torch.float32 or t.device != dev or not t.is_contiguous():
            raise ValueError("value_normalizer.%s must be a float32 tensor on %s (ValueNorm(1, device=...)): it is updated in place" % (n, dev))
    return st, float(getattr(vn, "beta", 0.99999)), float(getattr(vn, "epsilon", 1e-5))


def _column(name, t, rows, dev, dtypes=(torch.float32,)):
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s must be a tensor" % name)
    if t.dtype not in dtypes:
        raise ValueError("%s must be %s, not %s" % (name, " or ".join(str(d) for d in dtypes), t.dtype))
    if tuple(t.shape) not in ((rows, 1), (rows,)):
        if name == "actions" and t.dim() == 2 and t.shape[0] == rows:
            raise NotImplementedError("actions of shape %s: only a single Discrete head is supported (MultiDiscrete, mixed and continuous heads are not)"
                                      % (tuple(t.shape),))
        raise ValueError("%s must have shape (%d, 1), not %s" % (name, rows, tuple(t.shape)))
    if t.device != dev:
        raise ValueError("%s must be on %s (the device of logits)" % (name, dev))
    return t.detach().contiguous()


def _logits_shape(logits):
    """(device, rows, n_actions) of a policy head's logits [rows, n_actions], checked (sample_actions checks its logits here too)."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 2 or not logits.is_floating_point():
        raise ValueError("logits must be a floating-point tensor [rows, n_actions]")
    rows, K = int(logits.shape[0]), int(logits.shape[1])
    if rows < 1 or K < 1:
        raise ValueError("logits must have at least one row and one action")
    if K > _lib.PPO_MAX_ACTIONS:
        raise ValueError("n_actions = %d is above the supported %d" % (K, _lib.PPO_MAX_ACTIONS))
    return logits.device, rows, K


def _widened(t):
    return t.float() if t.dtype in (torch.float16, torch.bfloat16) else t


def _available(avail, rows, K, dev, contiguous=False):
    # contiguous=True refuses a strided one (sample_actions), else it is copied
    if not isinstance(avail, torch.Tensor) or avail.dtype != torch.float32 or tuple(avail.shape) != (rows, K):
        raise ValueError("available_actions must be a float32 tensor of shape (%d, %d) or None" % (rows, K))
    if contiguous and not avail.is_contiguous():
        raise ValueError("available_actions must be contiguous")
    if avail.device != dev:
        raise ValueError("available_actions must be on %s (the device of logits)" % dev)
    return avail.detach().contiguous()


def _minibatch(logits, other, other_name, sample, rows, K, dev):
    """What both entry points do with their inputs once their shapes are checked: logits and `other` (values or critic_features) widened to float32, the
    sample's five float32 columns, its actions and its available_actions (or None), each checked against logits."""
    logits, other = _widened(logits), _widened(other)
    if logits.dtype != torch.float32 or other.dtype != torch.float32:
        raise ValueError("logits and %s must be float32 (or float16 / bfloat16, widened here)" % other_name)
    f = _fields(sample)
    cols = {k: _column(k, f[k], rows, dev) for k in ("value_preds", "returns", "active_masks", "old_action_log_probs", "adv_targ")}
    actions = _column("actions", f["actions"], rows, dev, (torch.float32, torch.int64))
    avail = f["available_actions"]
    if avail is not None:
        avail = _available(avail, rows, K, dev)
    return logits, other, cols, actions, avail


def _bind_minibatch(plan, rows, K, flags, clip, delta, ent, cols, actions, avail):
    # the fields gmpe_ppo_loss_plan and gmpe_popart_loss_plan name alike
    plan.rows, plan.n_actions, plan.flags, plan.actions_int64 = rows, K, flags, int(actions.dtype == torch.int64)
    plan.clip_param, plan.huber_delta, plan.entropy_coef = clip, delta, ent
    plan.actions = actions.data_ptr()
    plan.available_actions = None if avail is None else avail.data_ptr()
    for k, t in cols.items():
        setattr(plan, k, t.data_ptr())


class _Attach(torch.autograd.Function):
    """A scalar the kernel computed from `x`, with its gradient d scalar / d x already known: backward multiplies it by the incoming scalar. The two
    losses are two such nodes, so each is backpropagated on its own, as ppo_update does."""

    @staticmethod
    def forward(ctx, x, scalar, grad):
        ctx.save_for_backward(grad)
        return scalar.clone()                          # owns its storage

    @staticmethod
    def backward(ctx, g):
        grad, = ctx.saved_tensors
        return grad * g, None, None


class _Call(object):
    """One minibatch bound to a gmpe_ppo_loss_plan: the plan, the tensors it points to (kept alive with it) and what the results are made from."""

    def __init__(self, logits, values, sample_or_fields, args, value_normalizer, workspace):
        flags, clip, delta, ent = _flags(args)
        dev, rows, K = _logits_shape(logits)
        if not isinstance(values, torch.Tensor) or not values.is_floating_point() or tuple(values.shape) not in ((rows, 1), (rows,)):
            raise ValueError("values must be a floating-point tensor of shape (%d, 1)" % rows)
        if values.device != dev:
            raise ValueError("values must be on %s (the device of logits)" % dev)
        logits, values, cols, actions, avail = _minibatch(logits, values, "values", sample_or_fields, rows, K, dev)
        state = None
        plan = _lib.GmpePpoLossPlan()
        if flags & _lib.PPO_VALUENORM:
            state, plan.beta, plan.epsilon = _valuenorm_state(value_normalizer, dev)
            plan.running_mean, plan.running_mean_sq, plan.debiasing_term = (t.data_ptr() for t in state)
        else:
            plan.beta, plan.epsilon = 0.99999, 1e-5
        _need_cuda(dev)
        workspace = _workspace(workspace_bytes(rows), workspace, dev)
        _bind_minibatch(plan, rows, K, flags, clip, delta, ent, cols, actions, avail)
        plan.workspace, plan.workspace_bytes = workspace.data_ptr(), workspace.numel()
        values2 = values if values.dim() == 2 else values.reshape(rows, 1)
        lg, vl = logits.detach().contiguous(), values2.detach().contiguous()
        out = torch.empty((_lib.PPO_NUM_OUT,), dtype=torch.float64, device=dev)
        grad_logits, grad_values = torch.empty_like(lg), torch.empty_like(vl)
        logp, ratio = (torch.empty((rows, 1), dtype=torch.float32, device=dev) for _ in range(2))
        plan.logits, plan.values, plan.out = lg.data_ptr(), vl.data_ptr(), out.data_ptr()
        plan.grad_logits, plan.grad_values = grad_logits.data_ptr(), grad_values.data_ptr()
        plan.action_log_probs, plan.imp_weights = logp.data_ptr(), ratio.data_ptr()
        # the inputs the plan points to live until the launches are enqueued on this stream
        self.keep = (cols, actions, avail, state, workspace, lg, vl)
        self.plan, self.dev, self.logits, self.values2, self.out = plan, dev, logits, values2, out
        self.grad_logits, self.grad_values, self.logp, self.ratio = grad_logits, grad_values, logp, ratio

    def losses(self, scale=1):
        """PPOLosses from `out` and the stored gradients; scale (reduce="mean"): the scalars and the gradients times the number of shards."""
        s = self.out.to(torch.float32)                     # doubles are written as doubles; rounded once here
        if scale != 1:
            s = s * scale
            self.grad_logits.mul_(scale)
            self.grad_values.mul_(scale)
        o = _lib.PPO_OUT.index
        return PPOLosses(_Attach.apply(self.logits, s[o("actor_loss")], self.grad_logits), _Attach.apply(self.values2, s[o("value_loss")], self.grad_values),
                         s[o("policy_loss")], s[o("dist_entropy")], s[o("ratio_mean")], self.logp, self.ratio)


def _reduce(reduce):
    if reduce not in ("sum", "mean"):
        raise ValueError("reduce must be 'sum' (shard contributions) or 'mean' (times world, for DDP's gradient average), not %r" % (reduce,))
    return reduce


def ppo_losses(logits, values, sample_or_fields, args, value_normalizer=None, workspace=None, shards=None, reduce="sum"):
    """actor_loss (policy_loss - entropy_coef * dist_entropy) and value_loss of GR_MAPPO.ppo_update for one minibatch, differentiable with respect to
    `logits` [rows, n_actions] (the policy head's linear output, before masking) and `values` [rows, 1]; policy_loss, dist_entropy, ratio_mean
    (imp_weights.mean()), action_log_probs and imp_weights come detached. sample_or_fields: the generators' 16-tuple as it comes out of
    DeviceRolloutBuffer.feed_forward_generator, or a dict with actions (float32 or int64), value_preds, returns, active_masks, old_action_log_probs,
    adv_targ and optionally available_actions. args: the runner's args (clip_param, huber_delta, entropy_coef, use_policy_active_masks,
    use_value_active_masks, use_clipped_value_loss, use_huber_loss, use_valuenorm, use_popart; the reference's defaults where absent).
    With use_valuenorm the ValueNorm's three tensors (on the device) are updated in place before the returns are normalised, as cal_value_loss does.
    f16 / bf16 logits and values are widened to float32 first. A zero sum of active_masks gives NaN losses, like the reference's 0 / 0; nothing here
    waits for the device. workspace: an optional uint8 device tensor of workspace_bytes(rows) to reuse between calls.
    shards: None, or the exchange of a data-parallel learner (gmpe.learner_shards): the rows are this rank's part of a minibatch whose other parts lie
    on the other ranks, and the means, the ValueNorm update and the gradients are those of the WHOLE minibatch — ppo_losses_begin,
    shards.exchange(.local), ppo_losses_finish(reduce=reduce). reduce is read with shards only."""
    _reduce(reduce)
    if shards is not None:
        from . import learner_shards
        learner_shards.check_shards(shards)
        h = ppo_losses_begin(logits, values, sample_or_fields, args, value_normalizer, workspace)
        return ppo_losses_finish(h, learner_shards.gather(shards, h.local, "ppo_losses"), reduce)
    c = _Call(logits, values, sample_or_fields, args, value_normalizer, workspace)
    _lib.check(_lib.load().gmpe_ppo_loss(_ordinal(c.dev), C.byref(c.plan), _stream_of(c.dev)), "gmpe_ppo_loss")
    return c.losses()


class PPOLossShard(object):
    """What ppo_losses_begin leaves for ppo_losses_finish: `.local`, this shard's (sum returns, sum returns^2, sum active_masks, rows) as an f64 [4]
    device tensor (valid once the stream reaches it), and the bound minibatch with everything its plan points to."""

    def __init__(self, call, plan, local):
        self.call, self.plan, self.local, self.done = call, plan, local, False

    @property
    def out(self):
        """The f64 [GMPE_PPO_NUM_OUT] row of the call (_lib.PPO_OUT names the columns), written by finish: this shard's contributions before any
        reduce="mean" scaling, and the global denominators in the two DENOM columns."""
        return self.call.out


def ppo_losses_begin(logits, values, sample_or_fields, args, value_normalizer=None, workspace=None):
    """The first phase of ppo_losses over one shard of a minibatch (gmpe_ppo_loss_shard, GMPE_SHARD_LOCAL), same arguments: the shard's double sums in
    ppo_losses' own merge order and its row count go to the handle's `.local`; the ValueNorm is not touched yet. -> PPOLossShard"""
    c = _Call(logits, values, sample_or_fields, args, value_normalizer, workspace)
    from . import learner_shards
    sp = _lib.GmpePpoLossShardPlan()
    local = learner_shards.begin("gmpe_ppo_loss_shard", sp, c.plan, _lib.PPO_SHARD_STATS, c.dev)
    return PPOLossShard(c, sp, local)


def ppo_losses_finish(handle, all_stats, reduce="sum"):
    """The second phase (GMPE_SHARD_APPLY): all_stats f64 [world, 4], row r = shard r's `.local` (torch.stack in one process, an all-gather across
    ranks), added in index order. The denominators, the ValueNorm update (every replica receives the same one) and the normalisation of the returns
    come from the sums over the WHOLE minibatch. reduce="sum": the scalars are this shard's contributions — over all shards they add up to the
    scalars of the whole minibatch — and backward() leaves the rows of the gradient of the global loss. reduce="mean": both times world, so that
    DDP's average over ranks is the global gradient. Once per handle. -> PPOLosses"""
    from . import learner_shards
    _reduce(reduce)
    if not isinstance(handle, PPOLossShard):
        raise TypeError("handle must come from ppo_losses_begin")
    c = handle.call
    world = learner_shards.finish("gmpe_ppo_loss_shard", handle, c.dev, all_stats, "ppo_losses_finish",
                                  "ppo_losses_finish was already called on this handle (it would update the ValueNorm twice)")
    return c.losses(world if reduce == "mean" else 1)


def popart_workspace_bytes(rows, hidden):
    """Device scratch (bytes) one ppo_losses_popart call over `rows` rows of `hidden` critic features needs (gmpe_ppo_loss_popart_workspace_bytes)."""
    n = C.c_size_t()
    _lib.check(_lib.load().gmpe_ppo_loss_popart_workspace_bytes(int(rows), int(hidden), C.byref(n)), "gmpe_ppo_loss_popart_workspace_bytes")
    return int(n.value)


def _popart_state(popart, hidden, dev):
    """The tensors of the reference's PopArt(hidden, 1) (onpolicy/algorithms/utils/popart.py:30-41), duck-typed: (weight, bias, stddev, mean, mean_sq,
    debiasing_term), beta, epsilon. Everything is checked before the device is touched."""
    if popart is None:
        raise ValueError("popart (the critic's v_out, a PopArt(hidden, 1)) is required")
    names = ("weight", "bias", "stddev", "mean", "mean_sq", "debiasing_term")
    for n in names:
        if not isinstance(getattr(popart, n, None), torch.Tensor):
            raise NotImplementedError("popart.%s is missing or no tensor: popart must be a PopArt (%s)" % (n, ", ".join(names)))
    if int(getattr(popart, "norm_axes", 1)) != 1:
        raise NotImplementedError("popart.norm_axes = %r: only norm_axes 1 is supported" % (popart.norm_axes,))
    if int(getattr(popart, "output_shape", 1)) != 1:
        raise NotImplementedError("popart.output_shape = %r: only PopArt(hidden, 1) is supported" % (popart.output_shape,))
    st = [getattr(popart, n) for n in names]
    if tuple(st[0].shape) != (1, hidden):
        if st[0].dim() == 2 and st[0].shape[0] > 1:
            raise NotImplementedError("popart.weight of shape %s: only PopArt(hidden, 1) is supported" % (tuple(st[0].shape),))
        raise ValueError("popart.weight must have shape (1, %d) (critic_features has %d columns), not %s" % (hidden, hidden, tuple(st[0].shape)))
    for n, t in zip(names[1:5], st[1:5]):
        if tuple(t.shape) != (1,):
            raise ValueError("popart.%s must have shape (1,), not %s" % (n, tuple(t.shape)))
    if st[5].numel() != 1:
        raise ValueError("popart.debiasing_term must hold one element, not %s" % (tuple(st[5].shape),))
    for n, t in zip(names, st):
        if t.dtype != torch.float32 or t.device != dev or not t.is_contiguous():
            raise ValueError("popart.%s must be a contiguous float32 tensor on %s (the device of logits): the kernel reads and writes it where it lies"
                             % (n, dev))
    return st, float(getattr(popart, "beta", 0.99999)), float(getattr(popart, "epsilon", 1e-5))


class _AttachHead(torch.autograd.Function):
    """value_loss as ONE node over (critic_features, weight, bias): the kernel evaluated v_out and left the three gradients; backward multiplies them
    by the incoming scalar. No tensor of the layer is saved, so rewriting the weight after the call is no hazard."""

    @staticmethod
    def forward(ctx, features, weight, bias, scalar, gf, gw, gb):
        ctx.save_for_backward(gf, gw, gb)
        return scalar.clone()

    @staticmethod
    def backward(ctx, g):
        gf, gw, gb = ctx.saved_tensors
        return gf * g, gw * g, gb * g, None, None, None, None


def ppo_losses_popart(logits, critic_features, sample_or_fields, args, popart, install="replace", workspace=None, shards=None):
    """ppo_losses for --use_popart, where trainer.value_normalizer is the critic's output layer v_out = PopArt(hidden, 1) (graph_mappo.py:63-64): the
    critic is called up to `critic_features` [rows, hidden] (the input of v_out), and one call of gmpe_ppo_loss_popart (four launches) does what
    evaluate_actions' last line and cal_value_loss do, in their order: values = F.linear(critic_features, weight, bias) with the weights as they are
    BEFORE the update; PopArt.update(returns) (popart.py:62-83: float32, all rows, stddev from the raw statistics, the bias through the aliased
    old_mean, i.e. ((stddev * b + mean') - mean') / stddev'); normalize(returns) with the debiased statistics; the losses; the gradients.
    popart: duck-typed — weight [1, hidden], bias, stddev, mean, mean_sq [1], debiasing_term (one element), float32, contiguous, on the device of
    logits; beta, epsilon (PopArt's defaults where absent); norm_axes == 1, output_shape == 1. mean, mean_sq and debiasing_term are updated in place.
    install="replace" (the reference): popart.weight, .bias and .stddev become NEW nn.Parameters holding the rescaled layer; the objects that were
    there at the call receive this minibatch's gradients, and an optimiser built over them keeps them — it never trains the new ones.
    install="in_place": the rescaled layer is written into the existing storage; the Parameters keep their identity and the optimiser trains them.
    Returns PPOPopArtLosses: the PPOLosses fields plus `values` (detached [rows, 1], what v_out gave with the pre-update weights). value_loss is one
    autograd node over (critic_features, the weight and bias objects of the call); actor_loss is as in ppo_losses. f16 / bf16 logits and features
    are widened to float32 first. Nothing here waits for the device. workspace: an optional uint8 device tensor of popart_workspace_bytes(rows, hidden).
    shards: must be None — the sharded form (ppo_losses(..., shards=...)) does not cover PopArt."""
    if shards is not None:
        raise NotImplementedError("ppo_losses_popart(shards=...): the PopArt variant has no sharded form (gmpe_ppo_loss_shard covers ValueNorm or no "
                                  "normaliser); a data-parallel learner with --use_popart is not supported")
    flags, clip, delta, ent = _flags(args, popart=True)
    if install not in ("replace", "in_place"):
        raise ValueError("install must be 'replace' (the reference: new Parameters) or 'in_place', not %r" % (install,))
    dev, rows, K = _logits_shape(logits)
    if not isinstance(critic_features, torch.Tensor) or not critic_features.is_floating_point() or critic_features.dim() != 2 or \
            critic_features.shape[0] != rows or critic_features.shape[1] < 1:
        raise ValueError("critic_features must be a floating-point tensor of shape (%d, hidden)" % rows)
    H = int(critic_features.shape[1])
    if H > _lib.POPART_MAX_HIDDEN:
        raise ValueError("hidden = %d is above the supported %d" % (H, _lib.POPART_MAX_HIDDEN))
    if critic_features.device != dev:
        raise ValueError("critic_features must be on %s (the device of logits)" % dev)
    logits, critic_features, cols, actions, avail = _minibatch(logits, critic_features, "critic_features", sample_or_fields, rows, K, dev)
    (w_obj, b_obj, s_obj, mean, mean_sq, debias), beta, epsilon = _popart_state(popart, H, dev)
    _need_cuda(dev)
    workspace = _workspace(popart_workspace_bytes(rows, H), workspace, dev)
    lg, ft = logits.detach().contiguous(), critic_features.detach().contiguous()
    if install == "replace":
        w_out, b_out, s_out = torch.empty_like(w_obj.detach()), torch.empty_like(b_obj.detach()), torch.empty_like(s_obj.detach())
    else:
        w_out, b_out, s_out = w_obj, b_obj, s_obj                       # the aliasing case of the C contract: written after the rows have read them
    out = torch.empty((_lib.PPO_NUM_OUT,), dtype=torch.float64, device=dev)
    grad_logits, grad_features = torch.empty_like(lg), torch.empty_like(ft)
    grad_weight, grad_bias = torch.empty_like(w_obj.detach()), torch.empty_like(b_obj.detach())
    logp, ratio, values = (torch.empty((rows, 1), dtype=torch.float32, device=dev) for _ in range(3))
    plan = _lib.GmpePopartLossPlan()
    _bind_minibatch(plan, rows, K, flags, clip, delta, ent, cols, actions, avail)
    plan.hidden, plan.beta, plan.epsilon = H, beta, epsilon
    plan.logits, plan.critic_features = lg.data_ptr(), ft.data_ptr()
    plan.weight, plan.bias, plan.stddev = w_obj.data_ptr(), b_obj.data_ptr(), s_obj.data_ptr()
    plan.mean, plan.mean_sq, plan.debiasing_term = mean.data_ptr(), mean_sq.data_ptr(), debias.data_ptr()
    plan.weight_out, plan.bias_out, plan.stddev_out = w_out.data_ptr(), b_out.data_ptr(), s_out.data_ptr()
    plan.values_out, plan.out = values.data_ptr(), out.data_ptr()
    plan.grad_logits, plan.grad_features, plan.grad_weight, plan.grad_bias = (t.data_ptr() for t in (grad_logits, grad_features, grad_weight, grad_bias))
    plan.action_log_probs, plan.imp_weights = logp.data_ptr(), ratio.data_ptr()
    plan.workspace, plan.workspace_bytes = workspace.data_ptr(), workspace.numel()
    _lib.check(_lib.load().gmpe_ppo_loss_popart(_ordinal(dev), C.byref(plan), _stream_of(dev)), "gmpe_ppo_loss_popart")
    s = out.to(torch.float32)
    o = _lib.PPO_OUT.index
    actor = _Attach.apply(logits, s[o("actor_loss")], grad_logits)
    value = _AttachHead.apply(critic_features, w_obj, b_obj, s[o("value_loss")], grad_features, grad_weight, grad_bias)
    if install == "replace":                                            # popart.py:79-83: three new nn.Parameter objects
        popart.stddev = torch.nn.Parameter(s_out)
        popart.weight = torch.nn.Parameter(w_out)
        popart.bias = torch.nn.Parameter(b_out)
    return PPOPopArtLosses(actor, value, s[o("policy_loss")], s[o("dist_entropy")], s[o("ratio_mean")], logp, ratio, values)
