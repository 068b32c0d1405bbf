"""The policy's action head on the device (include/gmpe.h gmpe_head_forward / gmpe_head_backward / gmpe_act_head): the Linear of the reference's
Categorical under a single Discrete ACTLayer (onpolicy/algorithms/utils/act.py:27-29, distributions.py:72-91), 64 -> n_actions <= 64.

    logits = gmpe.action_logits(actor_features, self.act)                 # was: self.act.action_out.linear(actor_features); training
    idx, actions, action_log_probs = gmpe.act_head(actor_features, self.act, available_actions, seed=..., num_agents=..., draw=step)      # a rollout

A torch GEMM picks its kernel, and so its summation order, by the batch shape; here a row's logits are one fixed fmaf chain, whatever the batch. With
that, the log-prob act_head stores in a rollout of 40 960 rows is bit for bit what ppo_losses recomputes from action_logits on a minibatch of any other
size: an unchanged policy has importance weights of exactly 1, end to end. There is no torch fallback: the arrays must be on a HIP device.
"""
import ctypes as C

import torch

from . import _layers, _lib, act as _act
from .engine import _need_cuda, _ordinal, _stream_of

HIDDEN = 64                                             # the hidden size the library is built for
MAX_ACTIONS = 64                                        # GMPE_PPO_MAX_ACTIONS


def head_workspace_bytes(rows, n_actions, backward=True):
    """Device scratch (bytes) one training action_logits call over `rows` rows needs (gmpe_head_workspace_bytes); 0 without backward."""
    if not 1 <= int(n_actions) <= MAX_ACTIONS:
        raise ValueError("n_actions = %d: the action head takes 1 .. %d actions" % (int(n_actions), MAX_ACTIONS))
    n = C.c_size_t()
    _lib.check(_lib.load().gmpe_head_workspace_bytes(int(rows), int(n_actions), int(bool(backward)), C.byref(n)), "gmpe_head_workspace_bytes")
    return int(n.value)


def _head_params(act, fn):
    """(weight, bias) of the head's Linear, duck-typed: the reference's ACTLayer (.action_out.linear), a Categorical (.linear) or an nn.Linear.
    What is not a single Discrete head is refused by name, in the name of the public function `fn`."""
    if getattr(act, "multi_discrete", False):
        raise NotImplementedError("act.multi_discrete is set: %s is built for a single Discrete head (MultiDiscrete is not supported)" % fn)
    if getattr(act, "mixed_action", False):
        raise NotImplementedError("act.mixed_action is set: %s is built for a single Discrete head (mixed action spaces are not supported)" % fn)
    if getattr(act, "action_outs", None) is not None:
        raise NotImplementedError("act.action_outs: %s is built for a single Discrete head (a list of heads is not supported)" % fn)
    path, dist = "act", act
    if getattr(act, "action_out", None) is not None:
        path, dist = "act.action_out", act.action_out
    kind = type(dist).__name__
    if kind in ("DiagGaussian", "Bernoulli") or hasattr(dist, "fc_mean") or hasattr(dist, "logstd"):
        raise NotImplementedError("%s is a %s: %s is built for a Categorical head (DiagGaussian and Bernoulli heads are not supported)" % (path, kind, fn))
    if getattr(dist, "linear", None) is not None:
        path, lin = path + ".linear", dist.linear
    elif isinstance(getattr(dist, "weight", None), torch.Tensor):
        lin = dist                                      # an nn.Linear
    else:
        raise ValueError("%s.linear is missing: act must be an ACTLayer (.action_out.linear), a Categorical (.linear) or an nn.Linear" % path)
    return path, _layers.tensor_attr(lin, path, "weight"), _layers.tensor_attr(lin, path, "bias")


def _check(fn, features, path, weight, bias):
    """Everything the host can see of the features and the parameters but where they lie -> (device, rows, K, the named tensors for _on_device)"""
    if not isinstance(features, torch.Tensor):
        raise ValueError("actor_features must be a tensor")
    tensors = [("actor_features", features), (path + ".weight", weight), (path + ".bias", bias)]
    _layers.need_float32(fn, tensors)
    if features.dim() != 2 or features.shape[0] < 1:
        raise ValueError("actor_features must have shape (rows, %d) with rows >= 1, not %s" % (HIDDEN, tuple(features.shape)))
    if weight.dim() != 2 or bias.dim() != 1 or weight.shape[0] < 1 or bias.shape[0] != weight.shape[0]:
        raise ValueError("%s.weight / .bias must have shapes (K, %d) and (K,), not %s and %s" % (path, HIDDEN, tuple(weight.shape), tuple(bias.shape)))
    if int(weight.shape[1]) != HIDDEN or int(features.shape[1]) != HIDDEN:
        raise NotImplementedError("H = %d (actor_features has %d columns): %s is built for hidden = %d"
                                  % (int(weight.shape[1]), int(features.shape[1]), fn, HIDDEN))
    K = int(weight.shape[0])
    if K > MAX_ACTIONS:
        raise ValueError("K = %d actions: the action head takes at most %d" % (K, MAX_ACTIONS))
    if not features.is_contiguous():
        raise ValueError("actor_features must be contiguous")
    return features.device, int(features.shape[0]), K, tensors


def _on_device(tensors, dev):
    _need_cuda(dev)
    _layers.need_device(tensors, dev, "actor_features")


def _plan(rows, K, features, weight, bias):
    p = _lib.GmpeHeadPlan()
    p.rows, p.n_actions, p.hidden = rows, K, HIDDEN
    p.features, p.weight, p.bias = features.data_ptr(), weight.data_ptr(), bias.data_ptr()
    return p


class _Head(torch.autograd.Function):
    """logits = features W^T + b as one node over (features, weight, bias): forward one launch, backward at most three. Only the inputs are kept; the
    workspace is backward's own scratch."""

    @staticmethod
    def forward(ctx, rows, K, workspace, features, weight, bias):
        dev = features.device
        cs = [t.detach().contiguous() for t in (features, weight, bias)]
        logits = torch.empty((rows, K), dtype=torch.float32, device=dev)
        plan = _plan(rows, K, *cs)
        plan.logits_out = logits.data_ptr()
        _layers.run("gmpe_head_forward", dev, plan)
        if workspace is not None:
            ctx.save_for_backward(cs[0], cs[1])
        ctx.rows, ctx.K, ctx.workspace = rows, K, workspace
        return logits

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gl):
        features, weight = ctx.saved_tensors
        dev = features.device
        gl = gl.contiguous()
        need = ctx.needs_input_grad[3:6]
        gf = torch.empty_like(features) if need[0] else None
        gw = torch.empty_like(weight) if need[1] else None
        gb = torch.empty((ctx.K,), dtype=torch.float32, device=dev) if need[2] else None
        plan = _lib.GmpeHeadPlan()
        plan.rows, plan.n_actions, plan.hidden = ctx.rows, ctx.K, HIDDEN
        plan.features, plan.weight, plan.grad_logits = features.data_ptr(), weight.data_ptr(), gl.data_ptr()
        plan.grad_features = None if gf is None else gf.data_ptr()
        plan.grad_weight = None if gw is None else gw.data_ptr()
        plan.grad_bias = None if gb is None else gb.data_ptr()
        plan.workspace, plan.workspace_bytes = ctx.workspace.data_ptr(), ctx.workspace.numel()
        _layers.run("gmpe_head_backward", dev, plan)
        return None, None, None, gf, gw, gb


def action_logits(actor_features, act, workspace=None):
    """act.action_out.linear(actor_features) on the device -> logits [rows, K], one autograd node over (actor_features, weight, bias): forward is one
    launch, backward at most three. The result goes unchanged into ppo_losses, ppo_losses(..., shards=...) and ppo_losses_popart.
      actor_features: float32 [rows, 64], contiguous, on the device.
      act: duck-typed — the reference's ACTLayer (act.action_out.linear.weight / .bias), a Categorical (.linear) or an nn.Linear, weight [K <= 64, 64].
        The parameters are read from the module, so the optimiser and the checkpoints do not change. MultiDiscrete, mixed, DiagGaussian and
        Bernoulli heads, half precision and a hidden size other than 64 raise NotImplementedError by name; malformed input raises ValueError.
      workspace: an optional uint8 device tensor of head_workspace_bytes(rows, K) to reuse between calls — backward's scratch, so it belongs to one
        forward until that forward's backward has run.
    Under torch.no_grad(), or when nothing requires a gradient, the forward-only plan runs: no workspace, nothing saved. A row's logits are a function of
    that row and the parameters alone (one fmaf chain from the bias over the 64 columns ascending), so the rows may be chunked freely; the parameter
    gradients are double sums in an order that depends on `rows` alone. Nothing here waits for the device."""
    path, weight, bias = _head_params(act, "action_logits")
    dev, rows, K, tensors = _check("action_logits", actor_features, path, weight, bias)
    _on_device(tensors, dev)
    train = torch.is_grad_enabled() and any(t.requires_grad for t in (actor_features, weight, bias))
    workspace = _layers.backward_workspace(train, lambda: head_workspace_bytes(rows, K), workspace, dev)
    return _Head.apply(rows, K, workspace, actor_features, weight, bias)


@torch.no_grad()
def act_head(actor_features, act, available_actions=None, *, dones_prev=None, stop_action=None, seed, env_id_base=0, num_agents, draw, draw_dev=None,
             draw_inc=1, deterministic=False, out=None, stream=None):
    """ACTLayer.forward of a single Discrete head from the actor features, one launch (gmpe_act_head): sample_actions with the features and the head module
    in place of the logits, and the same returns — (action_idx int32 [rows], actions int64 [rows, 1], action_log_probs float32 [rows, 1]). The head's
    Linear runs inside the sampling launch; every output is bit for bit what sample_actions(action_logits(actor_features, act), ...) gives.
      actor_features, act: as for action_logits. Every other argument: as for sample_actions.
      out: as for sample_actions, and it may hold "logits", float32 with rows * n_actions elements, which then receives the logits."""
    path, weight, bias = _head_params(act, "act_head")
    dev, rows, K, tensors = _check("act_head", actor_features, path, weight, bias)
    plan, outs, given, keep = _act._plan(rows, K, dev, "actor_features", available_actions, dones_prev, stop_action, seed, env_id_base, num_agents, draw,
                                         draw_dev, draw_inc, deterministic, out, more_out={"logits": (torch.float32, rows * K)})
    _on_device(tensors, dev)
    cs = [t.detach().contiguous() for t in (weight, bias)]
    hp = _plan(rows, K, actor_features.detach(), *cs)
    if "logits" in given:
        hp.logits_out = given["logits"].data_ptr()
    st = C.c_void_p(stream.cuda_stream) if stream is not None else _stream_of(dev)
    _lib.check(_lib.load().gmpe_act_head(_ordinal(dev), C.byref(plan), C.byref(hp), st), "gmpe_act_head")
    del keep, cs
    return outs
