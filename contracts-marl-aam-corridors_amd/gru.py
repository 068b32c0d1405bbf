"""The policy's masked GRU layer on the device (include/gmpe.h gmpe_gru_forward / gmpe_gru_backward): RNNLayer.forward
(onpolicy/algorithms/utils/rnn.py:23-79) as one launch, its backward as three, whatever the number of steps, of rows and the masks.

    actor_features, rnn_states = gmpe.rnn_layer(actor_features, rnn_states, masks, self.rnn)          # was: self.rnn(actor_features, rnn_states, masks)

The reference finds the steps with a zero mask on the host (a synchronisation per minibatch) and loops over the segments; here every row carries its own
mask through the recurrence. There is no torch fallback: the arrays must be on a HIP device.
"""
import ctypes as C

import torch

from . import _layers, _lib
from .engine import _need_cuda

SUPPORTED = ((64, 64),)                                 # (in_dim, hidden) the library is built for
_PARAMS = ("weight_ih", "weight_hh", "bias_ih", "bias_hh", "ln_weight", "ln_bias")


def rnn_workspace_bytes(L, Nb, H, backward=True):
    """Device scratch (bytes) one rnn_layer call over L steps of Nb rows with hidden size H needs (gmpe_gru_workspace_bytes); 0 without backward."""
    if (int(H), int(H)) not in SUPPORTED:
        raise NotImplementedError("hidden = %d: rnn_layer is built for (in_dim, hidden) in %s" % (int(H), list(SUPPORTED)))
    n = C.c_size_t()
    _lib.check(_lib.load().gmpe_gru_workspace_bytes(int(L), int(Nb), int(H), int(bool(backward)), C.byref(n)), "gmpe_gru_workspace_bytes")
    return int(n.value)


def _layer_params(layer):
    """The six tensors and eps of an RNNLayer, duck-typed: .rnn.weight_ih_l0 / weight_hh_l0 / bias_ih_l0 / bias_hh_l0, .norm.weight / bias / eps."""
    n = int(getattr(layer, "_recurrent_N", 1))
    if n != 1:
        raise NotImplementedError("recurrent_N = %d: rnn_layer supports a single GRU layer (recurrent_N == 1)" % n)
    rnn, norm = getattr(layer, "rnn", None), getattr(layer, "norm", None)
    if rnn is None or norm is None:
        raise ValueError("layer must have .rnn (the nn.GRU's weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0) and .norm (weight, bias, eps)")
    if getattr(rnn, "weight_ih_l1", None) is not None or bool(getattr(rnn, "bidirectional", False)):
        raise NotImplementedError("layer.rnn has more than one layer or direction: rnn_layer supports recurrent_N == 1, one direction")
    ps = []
    for owner, obj, names in (("rnn", rnn, ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")), ("norm", norm, ("weight", "bias"))):
        ps += [_layers.tensor_attr(obj, "layer." + owner, k) for k in names]
    return ps, float(getattr(norm, "eps", 1e-5))


def _check(x, hxs, masks, ps):
    """Everything the host can see, before the device is touched -> (device, L, Nb, D, H)"""
    for name, t in (("x", x), ("hxs", hxs), ("masks", masks)):
        if not isinstance(t, torch.Tensor):
            raise ValueError("%s must be a tensor" % name)
    tensors = (("x", x), ("hxs", hxs), ("masks", masks)) + tuple(zip(_PARAMS, ps))
    _layers.need_float32("rnn_layer", tensors)
    if x.dim() != 2 or hxs.dim() != 3 or hxs.shape[0] < 1 or x.shape[0] < 1:
        raise ValueError("x must have shape (L * Nb, D) and hxs (Nb, recurrent_N, H), not %s and %s" % (tuple(x.shape), tuple(hxs.shape)))
    if hxs.shape[1] != 1:
        raise NotImplementedError("hxs of shape %s: rnn_layer supports recurrent_N == 1" % (tuple(hxs.shape),))
    Nb, H, D = int(hxs.shape[0]), int(hxs.shape[2]), int(x.shape[1])
    if x.shape[0] % Nb:
        raise ValueError("x has %d rows, which is no multiple of the %d rows of hxs" % (x.shape[0], Nb))
    L = int(x.shape[0]) // Nb
    if tuple(masks.shape) not in ((L * Nb, 1), (L * Nb,)):
        raise ValueError("masks must have shape (%d, 1), not %s" % (L * Nb, tuple(masks.shape)))
    shapes = ((3 * H, D), (3 * H, H), (3 * H,), (3 * H,), (H,), (H,))
    for name, t, s in zip(_PARAMS, ps, shapes):
        if tuple(t.shape) != s:
            raise ValueError("layer's %s must have shape %s (x has %d columns, hxs %d), not %s" % (name, s, D, H, tuple(t.shape)))
    if (D, H) not in SUPPORTED:
        raise NotImplementedError("(in_dim, hidden) = (%d, %d): rnn_layer is built for %s" % (D, H, list(SUPPORTED)))
    dev = x.device
    _need_cuda(dev)
    _layers.need_device(tensors, dev, "x")
    return dev, L, Nb, D, H


def _plan(L, Nb, D, H, eps, x, hxs, masks, ps, features, hxs_out, workspace):
    p = _lib.GmpeGruPlan()
    p.steps, p.rows, p.in_dim, p.hidden, p.eps = L, Nb, D, H, eps
    p.x, p.hxs, p.masks = x.data_ptr(), hxs.data_ptr(), masks.data_ptr()
    for k, t in zip(_PARAMS, ps):
        setattr(p, k, t.data_ptr())
    if features is not None:
        p.features, p.hxs_out = features.data_ptr(), hxs_out.data_ptr()
    if workspace is not None:
        p.workspace, p.workspace_bytes = workspace.data_ptr(), workspace.numel()
    return p


class _Layer(torch.autograd.Function):
    """features, hxs_out = layer(x, hxs; masks) as one node over x, hxs and the six parameters. The workspace gmpe_gru_forward filled and the inputs
    are kept for gmpe_gru_backward; changing any of them in place between the two calls is the caller's error, as with any saved tensor."""

    @staticmethod
    def forward(ctx, x, hxs, w_ih, w_hh, b_ih, b_hh, ln_w, ln_b, masks, eps, dims, workspace):
        L, Nb, D, H = dims
        dev = x.device
        ps = [t.detach().contiguous() for t in (w_ih, w_hh, b_ih, b_hh, ln_w, ln_b)]
        xc, hc, mc = x.detach().contiguous(), hxs.detach().contiguous(), masks.detach().contiguous()
        features = torch.empty((L * Nb, H), dtype=torch.float32, device=dev)
        hxs_out = torch.empty((Nb, 1, H), dtype=torch.float32, device=dev)
        plan = _plan(L, Nb, D, H, eps, xc, hc, mc, ps, features, hxs_out, workspace)
        _layers.run("gmpe_gru_forward", dev, plan)
        ctx.save_for_backward(xc, hc, mc, *ps)
        ctx.workspace, ctx.eps, ctx.dims = workspace, eps, dims
        return features, hxs_out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gf, gh):
        xc, hc, mc = ctx.saved_tensors[:3]
        ps = list(ctx.saved_tensors[3:])
        L, Nb, D, H = ctx.dims
        dev = xc.device
        gf = torch.zeros((L * Nb, H), dtype=torch.float32, device=dev) if gf is None else gf.contiguous()
        grads = [torch.empty_like(t) for t in [xc, hc] + ps]
        plan = _plan(L, Nb, D, H, ctx.eps, xc, hc, mc, ps, None, None, ctx.workspace)       # backward neither reads nor writes features and hxs_out
        plan.grad_features = gf.data_ptr()
        if gh is not None:
            gh = gh.contiguous()
            plan.grad_hxs_out = gh.data_ptr()
        for k, t in zip(("grad_x", "grad_hxs") + tuple("grad_" + n for n in _PARAMS), grads):
            setattr(plan, k, t.data_ptr())
        _layers.run("gmpe_gru_backward", dev, plan)
        return tuple(grads) + (None, None, None, None)


def rnn_layer(x, hxs, masks, layer, workspace=None):
    """RNNLayer.forward(x, hxs, masks) of `layer` on the device -> (features [L * Nb, H], hxs_out [Nb, 1, H]), L = x.shape[0] // hxs.shape[0].
    x [L * Nb, D] time-major (row l * Nb + k, as recurrent_generator hands it out), hxs [Nb, 1, H], masks [L * Nb, 1] with values in {0, 1}: for every
    row on its own, h <- h * mask before each GRU step, features = LayerNorm(h), hxs_out = the last h. For 0 / 1 masks that is the reference's segment
    loop; L == 1 is its rollout branch. Masks outside {0, 1} are undefined (in the reference their effect depends on the other rows) and not checked.
    layer: duck-typed — .rnn.weight_ih_l0 / weight_hh_l0 / bias_ih_l0 / bias_hh_l0, .norm.weight / bias / eps and optionally _recurrent_N; the
    reference's RNNLayer works unchanged. Gradients reach x, hxs and the six parameters through one autograd node (three launches). Under
    torch.no_grad(), or when nothing requires a gradient, the forward-only plan runs: no workspace, nothing saved.
    float32 only, (in_dim, hidden) = (64, 64), recurrent_N == 1; everything else is refused by name before any launch. Nothing here waits for the
    device. workspace: an optional uint8 device tensor of rnn_workspace_bytes(L, Nb, H) to reuse between calls — it holds what backward needs, so it
    belongs to one forward until that forward's backward has run."""
    ps, eps = _layer_params(layer)
    dev, L, Nb, D, H = _check(x, hxs, masks, ps)
    train = torch.is_grad_enabled() and any(t.requires_grad for t in [x, hxs] + ps)
    workspace = _layers.backward_workspace(train, lambda: rnn_workspace_bytes(L, Nb, H), workspace, dev)
    return _Layer.apply(x, hxs, *ps, masks, eps, (L, Nb, D, H), workspace)
