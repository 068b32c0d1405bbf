"""The critic's value head on the device (include/gmpe.h gmpe_value_forward / gmpe_value_backward): v_out of the reference's GR_Critic
(onpolicy/algorithms/graph_actor_critic.py:395), 64 -> 1.

    values = gmpe.value_head(critic_features, self.v_out)                  # was: self.v_out(critic_features)
    gmpe.value_head(critic_features, self.v_out, out=buffer.value_preds[t])   # a rollout, under torch.no_grad()

A torch GEMM picks its kernel, and so its summation order, by the batch shape; here a row's value is one fixed dot product, whatever the batch — the one
ppo_losses_popart evaluates in training. With that, the value_preds a rollout of 40 960 rows stores are bit for bit what the PopArt loss recomputes on a
minibatch of any other size: for an unchanged critic the value clip sees values - value_preds == 0. There is no torch fallback: the arrays must be on a HIP
device.
"""
import ctypes as C

import torch

from . import _layers, _lib
from .engine import _need_cuda

HIDDEN = 64                                             # the hidden size the library is built for


def value_workspace_bytes(rows, backward=True):
    """Device scratch (bytes) one training value_head call over `rows` rows needs (gmpe_value_workspace_bytes); 0 without backward."""
    n = C.c_size_t()
    _lib.check(_lib.load().gmpe_value_workspace_bytes(int(rows), int(bool(backward)), C.byref(n)), "gmpe_value_workspace_bytes")
    return int(n.value)


def _check(features, v_out):
    """Everything the host can see of the features and the parameters but where they lie -> (weight, bias, rows, the named tensors for need_device)"""
    fn = "value_head"
    weight, bias = _layers.tensor_attr(v_out, "v_out", "weight"), _layers.tensor_attr(v_out, "v_out", "bias")
    if not isinstance(features, torch.Tensor):
        raise ValueError("critic_features must be a tensor")
    tensors = [("critic_features", features), ("v_out.weight", weight), ("v_out.bias", bias)]
    _layers.need_float32(fn, tensors)
    if features.dim() != 2 or features.shape[0] < 1:
        raise ValueError("critic_features must have shape (rows, %d) with rows >= 1, not %s" % (HIDDEN, tuple(features.shape)))
    if weight.dim() != 2 or bias.dim() != 1 or weight.shape[0] < 1 or bias.shape[0] != weight.shape[0]:
        raise ValueError("v_out.weight / .bias must have shapes (1, %d) and (1,), not %s and %s" % (HIDDEN, tuple(weight.shape), tuple(bias.shape)))
    if int(weight.shape[0]) != 1:
        raise NotImplementedError("v_out has %d output rows: %s is built for one value per row" % (int(weight.shape[0]), fn))
    if int(weight.shape[1]) != HIDDEN or int(features.shape[1]) != HIDDEN:
        raise NotImplementedError("H = %d (critic_features has %d columns): %s is built for hidden = %d"
                                  % (int(weight.shape[1]), int(features.shape[1]), fn, HIDDEN))
    if not features.is_contiguous():
        raise ValueError("critic_features must be contiguous")
    return weight, bias, int(features.shape[0]), tensors


def _forward(rows, features, weight, bias, out):
    """the forward launch -> (values [rows, 1] — `out` where given —, the contiguous inputs the launch read)"""
    dev = features.device
    cs = [t.detach().contiguous() for t in (features, weight, bias)]
    values = torch.empty((rows, 1), dtype=torch.float32, device=dev) if out is None else out
    plan = _lib.GmpeValuePlan()
    plan.rows, plan.hidden = rows, HIDDEN
    plan.features, plan.weight, plan.bias, plan.values_out = cs[0].data_ptr(), cs[1].data_ptr(), cs[2].data_ptr(), values.data_ptr()
    _layers.run("gmpe_value_forward", dev, plan)
    return values.view(rows, 1), cs


class _Value(torch.autograd.Function):
    """values = features W^T + b as one node over (features, weight, bias): forward one launch, backward at most two. Only the inputs are kept; the
    workspace is backward's own scratch."""

    @staticmethod
    def forward(ctx, rows, workspace, features, weight, bias):
        values, cs = _forward(rows, features, weight, bias, None)
        ctx.save_for_backward(cs[0], cs[1])
        ctx.rows, ctx.workspace = rows, workspace
        return values

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gv):
        features, weight = ctx.saved_tensors
        dev = features.device
        gv = gv.contiguous()
        need = ctx.needs_input_grad[2:5]
        gf = torch.empty_like(features) if need[0] else None
        gw = torch.empty_like(weight) if need[1] else None
        gb = torch.empty((1,), dtype=torch.float32, device=dev) if need[2] else None
        plan = _lib.GmpeValuePlan()
        plan.rows, plan.hidden = ctx.rows, HIDDEN
        plan.features, plan.weight, plan.grad_values = features.data_ptr(), weight.data_ptr(), gv.data_ptr()
        plan.grad_features = None if gf is None else gf.data_ptr()
        plan.grad_weight = None if gw is None else gw.data_ptr()
        plan.grad_bias = None if gb is None else gb.data_ptr()
        plan.workspace, plan.workspace_bytes = ctx.workspace.data_ptr(), ctx.workspace.numel()
        _layers.run("gmpe_value_backward", dev, plan)
        return None, None, gf, gw, gb


def value_head(critic_features, v_out, out=None, workspace=None):
    """v_out(critic_features) on the device -> values [rows, 1], one autograd node over (critic_features, weight, bias): forward is one launch, backward
    at most two.
      critic_features: float32 [rows, 64], contiguous, on the device.
      v_out: duck-typed — an nn.Linear(64, 1) or the reference's PopArt(64, 1): weight [1, 64], bias [1]. The parameters are read from the module, so the
        optimiser and the checkpoints do not change. Half precision, a hidden size other than 64 and more than one output row raise
        NotImplementedError by name; malformed input raises ValueError; all of it before the device is touched.
      out: an optional float32 device tensor of `rows` elements, contiguous — e.g. a rollout buffer's value_preds[t] — written in place and returned.
        Allowed only where no gradient is recorded: under torch.no_grad(), or when nothing requires one.
      workspace: an optional uint8 device tensor of value_workspace_bytes(rows) to reuse between calls — backward's scratch, so it belongs to one forward
        until that forward's backward has run.
    Under torch.no_grad(), or when nothing requires a gradient, the forward-only plan runs: no workspace, nothing saved. A row's value is a function of
    that row and the parameters alone — the dot product ppo_losses_popart evaluates, bit for bit —, so the rows may be chunked freely; the parameter
    gradients are double sums in an order that depends on `rows` alone. Nothing here waits for the device."""
    weight, bias, rows, tensors = _check(critic_features, v_out)
    dev = critic_features.device
    train = torch.is_grad_enabled() and any(t.requires_grad for t in (critic_features, weight, bias))
    if out is not None:
        if train:
            raise ValueError("out is written in place: it is allowed only without gradients (torch.no_grad(), or nothing that requires one)")
        if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.numel() != rows or not out.is_contiguous():
            raise ValueError("out must be a contiguous float32 tensor with %d elements" % rows)
        tensors = tensors + [("out", out)]
    _need_cuda(dev)
    _layers.need_device(tensors, dev, "critic_features")
    workspace = _layers.backward_workspace(train, lambda: value_workspace_bytes(rows), workspace, dev)
    if not train:
        return _forward(rows, critic_features, weight, bias, out)[0]
    return _Value.apply(rows, workspace, critic_features, weight, bias)
