"""The policy's MLPBase on the device (include/gmpe.h gmpe_mlp_forward / gmpe_mlp_backward): MLPBase.forward (onpolicy/algorithms/utils/mlp.py:44-76)
over the parts of its input as one launch, its backward as three, whatever the number of rows, of input columns, of hidden layers and of parts.

    actor_features = gmpe.mlp_base((obs, nbd_features), self.base)          # was: self.base(torch.cat([obs, nbd_features], dim=1))

The parts' columns are read as if concatenated; the concatenation is never written, and every part gets a gradient tensor of its own. There is no torch
fallback: the arrays must be on a HIP device.
"""
import ctypes as C

import torch

from . import _layers, _lib
from .engine import _need_cuda

HIDDEN = 64                                             # the hidden size the library is built for
MAX_LAYER_N, MAX_IN, MAX_PARTS = _lib.MLP_MAX_LAYERS - 1, _lib.MLP_MAX_IN, _lib.MLP_MAX_PARTS
_ACTIVATIONS = {"ReLU": _lib.MLP_RELU, "Tanh": _lib.MLP_TANH}
_LAYER = ("weight", "bias", "ln_weight", "ln_bias")


def mlp_workspace_bytes(rows, in_dim, layer_N=1, hidden=HIDDEN, backward=True):
    """Device scratch (bytes) one training mlp_base call over `rows` rows of `in_dim` columns needs (gmpe_mlp_workspace_bytes); 0 without backward."""
    if int(hidden) != HIDDEN:
        raise NotImplementedError("hidden = %d: mlp_base is built for hidden = %d" % (int(hidden), HIDDEN))
    if not 0 <= int(layer_N) <= MAX_LAYER_N:
        raise NotImplementedError("layer_N = %d: mlp_base is built for layer_N in 0 .. %d" % (int(layer_N), MAX_LAYER_N))
    if int(in_dim) > MAX_IN:
        raise NotImplementedError("D_in = %d: mlp_base is built for at most %d input columns" % (int(in_dim), MAX_IN))
    n = C.c_size_t()
    _lib.check(_lib.load().gmpe_mlp_workspace_bytes(int(rows), int(in_dim), int(hidden), int(layer_N), int(bool(backward)), C.byref(n)),
               "gmpe_mlp_workspace_bytes")
    return int(n.value)


def _block(owner, seq, names, ps, epss):
    """one nn.Sequential(Linear, activation, LayerNorm), duck-typed -> its activation's class name; appends its four tensors and its eps"""
    try:
        lin, act, norm = seq[0], seq[1], seq[2]
    except (TypeError, IndexError, KeyError):
        raise ValueError("base.mlp.%s must hold [0] the Linear, [1] the activation and [2] the LayerNorm" % owner)
    for obj, what, k in ((lin, "[0]", "weight"), (lin, "[0]", "bias"), (norm, "[2]", "weight"), (norm, "[2]", "bias")):
        ps.append(_layers.tensor_attr(obj, "base.mlp." + owner + what, k))
    names += ["%s.%s" % (owner, k) for k in _LAYER]
    epss.append(float(getattr(norm, "eps", 1e-5)))
    return type(act).__name__


def _base_params(base):
    """(names, tensors, meta) of an MLPBase, duck-typed: ._use_feature_normalization, .feature_norm (weight, bias, eps), .mlp.fc1, .mlp.fc2[i] for
    i < .mlp._layer_N. meta = (layer_N, activation, feature_norm, fn_eps, (eps per layer))."""
    mlp = getattr(base, "mlp", None)
    if mlp is None or getattr(mlp, "fc1", None) is None:
        raise ValueError("base must have .mlp with .fc1 (and .fc2, ._layer_N): the reference's MLPBase")
    layer_n = int(getattr(mlp, "_layer_N", 0))
    if layer_n < 0:
        raise ValueError("base.mlp._layer_N = %d must be >= 0" % layer_n)
    if layer_n > MAX_LAYER_N:
        raise NotImplementedError("layer_N = %d: mlp_base is built for layer_N in 0 .. %d" % (layer_n, MAX_LAYER_N))
    fc2 = getattr(mlp, "fc2", None) if layer_n else ()
    if layer_n and (fc2 is None or len(fc2) < layer_n):
        raise ValueError("base.mlp.fc2 holds %d layers, fewer than layer_N = %d" % (0 if fc2 is None else len(fc2), layer_n))
    names, ps, epss = [], [], []
    fnorm, fn_eps = bool(getattr(base, "_use_feature_normalization", False)), 1e-5
    if fnorm:
        norm = getattr(base, "feature_norm", None)
        for k in ("weight", "bias"):
            ps.append(_layers.tensor_attr(norm, "base.feature_norm", k, " (base._use_feature_normalization is set)"))
            names.append("feature_norm." + k)
        fn_eps = float(getattr(norm, "eps", 1e-5))
    acts = [_block("fc1", mlp.fc1, names, ps, epss)] + [_block("fc2[%d]" % i, fc2[i], names, ps, epss) for i in range(layer_n)]
    for a in acts:
        if a not in _ACTIVATIONS:
            raise NotImplementedError("activation %s: mlp_base is built for ReLU and Tanh" % a)
    if len(set(acts)) != 1:
        raise NotImplementedError("activations %s: mlp_base is built for one activation in every layer" % acts)
    return names, ps, (layer_n, _ACTIVATIONS[acts[0]], int(fnorm), fn_eps, tuple(epss))


def _check(parts, names, ps, meta):
    """Everything the host can see, before the device is touched -> (device, rows, dims)"""
    if len(parts) < 1:
        raise ValueError("parts must hold at least one tensor")
    if len(parts) > MAX_PARTS:
        raise NotImplementedError("%d parts: mlp_base is built for at most %d" % (len(parts), MAX_PARTS))
    for i, t in enumerate(parts):
        if not isinstance(t, torch.Tensor):
            raise ValueError("parts[%d] must be a tensor" % i)
    tensors = [("parts[%d]" % i, t) for i, t in enumerate(parts)] + list(zip(names, ps))
    _layers.need_float32("mlp_base", tensors)
    for i, t in enumerate(parts):
        if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError("parts[%d] must have shape (rows, d) with rows, d >= 1, not %s" % (i, tuple(t.shape)))
        if t.shape[0] != parts[0].shape[0]:
            raise ValueError("parts[%d] has %d rows, parts[0] has %d" % (i, t.shape[0], parts[0].shape[0]))
    rows, dims = int(parts[0].shape[0]), tuple(int(t.shape[1]) for t in parts)
    D, (layer_n, _, fnorm, _, _) = sum(dims), meta
    hidden = int(ps[2 * fnorm].shape[0]) if ps[2 * fnorm].dim() == 2 else -1
    if hidden > 0 and hidden != HIDDEN:
        raise NotImplementedError("hidden = %d: mlp_base is built for hidden = %d" % (hidden, HIDDEN))
    if D > MAX_IN:
        raise NotImplementedError("D_in = %d: mlp_base is built for at most %d input columns" % (D, MAX_IN))
    shapes = [(D,), (D,)] * fnorm + [(HIDDEN, D), (HIDDEN,), (HIDDEN,), (HIDDEN,)] + [(HIDDEN, HIDDEN), (HIDDEN,), (HIDDEN,), (HIDDEN,)] * layer_n
    for name, t, s in zip(names, ps, shapes):
        if tuple(t.shape) != s:
            raise ValueError("base's %s must have shape %s (the parts have %d columns), not %s" % (name, s, D, tuple(t.shape)))
    dev = parts[0].device
    _need_cuda(dev)
    _layers.need_device(tensors, dev, "parts[0]")
    return dev, rows, dims


def _plan(rows, dims, meta, parts, ps):
    layer_n, act, fnorm, fn_eps, epss = meta
    p = _lib.GmpeMlpPlan()
    p.rows, p.hidden, p.layer_n, p.activation, p.feature_norm, p.n_parts = rows, HIDDEN, layer_n, act, fnorm, len(parts)
    for i, t in enumerate(parts):
        p.part[i], p.part_dim[i] = t.data_ptr(), dims[i]
    if fnorm:
        p.fn_weight, p.fn_bias, p.fn_eps = ps[0].data_ptr(), ps[1].data_ptr(), fn_eps
    for l in range(layer_n + 1):
        for k, t in zip(_LAYER, ps[2 * fnorm + 4 * l:2 * fnorm + 4 * l + 4]):
            setattr(p.layer[l], k, t.data_ptr())
        p.layer[l].eps = epss[l]
    return p


def _grads_into(p, meta, gparts, gps):
    fnorm = meta[2]
    for i, t in enumerate(gparts):
        p.grad_part[i] = t.data_ptr()
    if fnorm:
        p.grad_fn_weight, p.grad_fn_bias = gps[0].data_ptr(), gps[1].data_ptr()
    for l in range(meta[0] + 1):
        for k, t in zip(_LAYER, gps[2 * fnorm + 4 * l:2 * fnorm + 4 * l + 4]):
            setattr(p.layer[l], "grad_" + k, t.data_ptr())


class _Base(torch.autograd.Function):
    """features = base(parts) as one node over the parts and all parameters. gmpe_mlp_backward recomputes a tile's forward, so only the inputs are kept;
    changing any of them in place before backward is the caller's error, as with any saved tensor. The workspace is backward's own scratch."""

    @staticmethod
    def forward(ctx, meta, rows, dims, workspace, *tensors):
        n = len(dims)
        dev = tensors[0].device
        cs = [t.detach().contiguous() for t in tensors]
        features = torch.empty((rows, HIDDEN), dtype=torch.float32, device=dev)
        plan = _plan(rows, dims, meta, cs[:n], cs[n:])
        plan.features = features.data_ptr()
        _layers.run("gmpe_mlp_forward", dev, plan)
        if workspace is not None:
            ctx.save_for_backward(*cs)
        ctx.meta, ctx.rows, ctx.dims, ctx.workspace = meta, rows, dims, workspace
        return features

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gf):
        cs, n = list(ctx.saved_tensors), len(ctx.dims)
        dev = cs[0].device
        gf = gf.contiguous()
        grads = [torch.empty_like(t) for t in cs]
        plan = _plan(ctx.rows, ctx.dims, ctx.meta, cs[:n], cs[n:])                  # backward neither reads nor writes features
        plan.grad_features = gf.data_ptr()
        plan.workspace, plan.workspace_bytes = ctx.workspace.data_ptr(), ctx.workspace.numel()
        _grads_into(plan, ctx.meta, grads[:n], grads[n:])
        _layers.run("gmpe_mlp_backward", dev, plan)
        return (None, None, None, None) + tuple(grads)


def mlp_base(parts, base, workspace=None):
    """MLPBase.forward(torch.cat(parts, dim=1)) of `base` on the device -> features [rows, 64].
    parts: one to four float32 device tensors [rows, d_i] (a single tensor stands for a 1-tuple) whose columns are read as if concatenated,
    1 <= sum d_i <= 256; the concatenation is never materialised and each part's gradient is a tensor of its own.
    base: duck-typed — ._use_feature_normalization and then .feature_norm (weight, bias, eps); .mlp.fc1 and .mlp.fc2[i], i < .mlp._layer_N, each
    [0] the Linear, [1] the activation (ReLU or Tanh, recognised from the class name), [2] the LayerNorm with its own eps. The reference's MLPBase works
    unchanged; the parameters are read from the module, so the optimiser and the checkpoints do not change. Gradients reach the parts and every
    parameter through one autograd node (three launches). Under torch.no_grad(), or when nothing requires a gradient, the forward-only plan runs: no
    workspace, nothing saved. float32 only, hidden = 64, layer_N in 0 .. 2; everything else is refused by name before any launch. Nothing here waits
    for the device. A row's result does not depend on the other rows, so the rows may be chunked freely.
    workspace: an optional uint8 device tensor of mlp_workspace_bytes(rows, sum d_i, layer_N) to reuse between calls — backward's scratch, so it belongs
    to one forward until that forward's backward has run."""
    if isinstance(parts, torch.Tensor):
        parts = (parts,)
    elif isinstance(parts, (tuple, list)):
        parts = tuple(parts)
    else:
        raise ValueError("parts must be a tensor or a tuple of tensors")
    names, ps, meta = _base_params(base)
    dev, rows, dims = _check(parts, names, ps, meta)
    train = torch.is_grad_enabled() and any(t.requires_grad for t in parts + tuple(ps))
    workspace = _layers.backward_workspace(train, lambda: mlp_workspace_bytes(rows, sum(dims), meta[0]), workspace, dev)
    return _Base.apply(meta, rows, dims, workspace, *parts, *ps)
