"""The gradient clip and the Adam step of GR_MAPPO.ppo_update on the device (include/gmpe.h gmpe_optim_step): nn.utils.clip_grad_norm_ followed by
torch.optim.Adam.step (onpolicy/algorithms/graph_mappo.py:212-227, :254-265) as two launches per 64 tensors, with nothing that waits for the device.

    grad_norm = gmpe.clip_and_step(optimizer, max_grad_norm, parameters=net.parameters())
    # was: grad_norm = nn.utils.clip_grad_norm_(net.parameters(), max_grad_norm); optimizer.step()

The optimiser stays the caller's unchanged torch.optim.Adam: its param_groups are read at every call, its state holds torch's own keys, so
optimizer.state_dict(), load_state_dict and a later optimizer.step() by torch keep working, in either order. There is no torch fallback: the tensors must
be on a HIP device.
"""
import ctypes as C
import struct

import torch

from . import _lib
from .engine import _need_cuda, _ordinal, _stream_of, _workspace

CHUNK = _lib.OPT_CHUNK
_TENSOR = struct.Struct("@PPPPqii")                 # gmpe_optim_tensor; tests/test_optim_host.py holds its size and _lib's layout to the header
_UNSUPPORTED = ("amsgrad", "maximize", "capturable", "differentiable", "decoupled_weight_decay")


def _number(group, gi, key, value):
    if isinstance(value, torch.Tensor):
        raise NotImplementedError("param_groups[%d][%r] is a tensor: clip_and_step takes Python numbers (a tensor hyper-parameter is not supported)" % (gi, key))
    return float(value)


def _groups(optimizer):
    """[(lr, beta1, beta2, eps, weight_decay)] per param_group of an Adam that clip_and_step can stand in for; everything else is refused by name"""
    if not isinstance(optimizer, torch.optim.Adam):
        raise NotImplementedError("optimizer is a %s: clip_and_step is built for torch.optim.Adam (other optimisers are not supported)"
                                  % type(optimizer).__name__)
    hypers = []
    for gi, g in enumerate(optimizer.param_groups):
        for key in _UNSUPPORTED:
            if g.get(key, False):
                raise NotImplementedError("param_groups[%d][%r] is set: clip_and_step is torch's plain single-tensor Adam (%s is not supported)"
                                          % (gi, key, key))
        if g.get("fused", None):
            raise NotImplementedError("param_groups[%d]['fused'] is True: its step counts live on the device; build the Adam without fused=True "
                                      "(fused is not supported)" % gi)
        b1, b2 = g["betas"]
        hypers.append((_number(g, gi, "lr", g["lr"]), _number(g, gi, "betas", b1), _number(g, gi, "betas", b2), _number(g, gi, "eps", g["eps"]),
                       _number(g, gi, "weight_decay", g["weight_decay"])))
    return hypers


_F32, _STRIDED = torch.float32, torch.strided


def _check_tensor(name, t, seen, numel=None):
    """a float32, contiguous, dense tensor; where it lies is judged once all are seen (`seen`: [(name, device)])"""
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s must be a tensor" % name)
    if t.is_sparse:
        raise NotImplementedError("%s is sparse: clip_and_step takes dense gradients (sparse gradients are not supported)" % name)
    if t.dtype in (torch.float16, torch.bfloat16):
        raise NotImplementedError("%s is %s: clip_and_step is float32 only (half precision is not supported)" % (name, t.dtype))
    if t.dtype != torch.float32:
        raise ValueError("%s must be float32, not %s" % (name, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    if numel is not None and t.numel() != numel:
        raise ValueError("%s must have %d elements, not %d" % (name, numel, t.numel()))
    seen.append((name, t.device))


def _judge(t, dev, numel, seen, name, *of):
    """_check_tensor behind its common case in one expression — this runs four times per tensor per call, and the host time is what the call is about;
    the name is formed only for a complaint"""
    if not (isinstance(t, torch.Tensor) and t.dtype is _F32 and t.layout is _STRIDED and t.is_contiguous() and t.numel() == numel and t.device == dev):
        _check_tensor(name % of, t, seen, numel)


def _table(optimizer, parameters, step):
    """The tensors of one call, before anything touches the device: [(tensor, flags, param_group index or None, state or None)] over the tensors that have
    a gradient — the optimiser's own in its order, then those of `parameters` alone — and the device. With step False the tensors that would only be
    stepped stay out and nothing is looked up in the state. Every refusal happens here."""
    hypers = _groups(optimizer)
    own = [(p, gi) for gi, g in enumerate(optimizer.param_groups) for p in g["params"]]
    if parameters is None:
        normed, extra = None, []
    else:
        plist = [parameters] if isinstance(parameters, torch.Tensor) else list(parameters)
        normed = {id(p) for p in plist}
        mine = {id(p) for p, _ in own}
        found, extra = set(), []
        for i, p in enumerate(plist):
            if not isinstance(p, torch.Tensor):
                raise ValueError("parameters[%d] must be a tensor" % i)
            if id(p) not in mine and id(p) not in found:
                found.add(id(p))
                extra.append((i, p))
    first = next((p for p in [p for p, _ in own] + [p for _, p in extra] if p.grad is not None), None)
    if first is None:                                   # no gradient anywhere: the device of the first tensor there is
        first = next(iter([p for p, _ in own] + [p for _, p in extra]), None)
        if first is None:
            raise ValueError("the optimiser and `parameters` hold no tensor")
    dev = first.device
    rows, seen = [], []                                 # seen: what _judge found unusual and _check_tensor let through, i.e. tensors that lie elsewhere
    for i, (p, gi) in enumerate(own):
        g = p.grad
        in_norm = normed is None or id(p) in normed
        if g is None or not (step or in_norm):
            continue
        n = p.numel()
        _judge(p, dev, n, seen, "param_groups[%d] parameter %d", gi, i)
        _judge(g, dev, n, seen, "param_groups[%d] parameter %d.grad", gi, i)
        if not step:
            rows.append((p, _lib.OPT_T_IN_NORM, None, None))
            continue
        st = optimizer.state[p]
        if st:
            t = st.get("step")
            if isinstance(t, torch.Tensor) and not t.is_cpu:
                raise NotImplementedError("param_groups[%d] parameter %d: the state's `step` is on %s; clip_and_step counts steps on the host, as a "
                                          "non-capturable, non-fused Adam does (capturable and fused state is not supported)" % (gi, i, t.device))
            _judge(st.get("exp_avg"), dev, n, seen, "param_groups[%d] parameter %d: state['exp_avg']", gi, i)
            _judge(st.get("exp_avg_sq"), dev, n, seen, "param_groups[%d] parameter %d: state['exp_avg_sq']", gi, i)
        rows.append((p, _lib.OPT_T_STEP | (_lib.OPT_T_IN_NORM if in_norm else 0), gi, st))
    for i, p in extra:
        if p.grad is None:
            continue
        _judge(p, dev, p.numel(), seen, "parameters[%d]", i)
        _judge(p.grad, dev, p.numel(), seen, "parameters[%d].grad", i)
        rows.append((p, _lib.OPT_T_IN_NORM, None, None))
    for name, d in seen:
        if d != dev:
            raise ValueError("%s is on %s: every tensor must be on %s (the device of the first one with a gradient)" % (name, d, dev))
    _need_cuda(dev)
    return hypers, rows, dev


def _new_state(st, p):
    """torch's lazy state initialisation of a non-capturable, non-fused Adam (Adam._init_group): `step` lives on the host"""
    st["step"] = torch.tensor(0.0, dtype=torch.float32)
    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)


def workspace_bytes(optimizer, parameters=None):
    """Device scratch (bytes) that is enough for any clip_and_step(optimizer, ..., parameters=parameters) call, whichever of the tensors have gradients:
    one double per chunk of 1024 elements, and a launch group's last chunk may be partial. gmpe_optim_workspace_bytes gives a plan's exact need."""
    tensors = {id(p): p for g in optimizer.param_groups for p in g["params"]}
    if parameters is not None:
        tensors.update((id(p), p) for p in ([parameters] if isinstance(parameters, torch.Tensor) else parameters))
    sizes = [int(p.numel()) for p in tensors.values() if p.numel() > 0]
    return 8 * (sum(sizes) // CHUNK + len(sizes))


@torch.no_grad()
def clip_and_step(optimizer, max_grad_norm=None, *, parameters=None, step=True, workspace=None):
    """nn.utils.clip_grad_norm_(parameters, max_grad_norm) followed by optimizer.step(), two launches per 64 tensors -> grad_norm, the total 2-norm as a
    0-dim float32 device tensor (formed in double, rounded once).
      optimizer: the caller's torch.optim.Adam, read through param_groups at this call (a changed lr is honoured; every group has its own lr, betas, eps,
        weight_decay). amsgrad, maximize, capturable, fused=True, differentiable, decoupled_weight_decay (AdamW), tensor hyper-parameters, half
        precision, sparse gradients and any optimiser that is not Adam raise NotImplementedError by name; CPU tensors, tensors on different devices,
        non-contiguous parameters, gradients or state and other dtypes raise ValueError — all before anything touches the device.
      max_grad_norm: None reports the norm and leaves the gradients bit for bit (the reference's get_grad_norm branch); a positive number scales the
        gradients of `parameters` by min(1, max_grad_norm / (norm + 1e-6)) in place, as torch does (also when the factor is 1).
      parameters: the tensors whose norm is taken and whose gradients are scaled; default: the optimiser's own. The two sets may differ (after a PopArt
        update with install="replace" critic.parameters() holds new tensors and the optimiser the old ones): a tensor of the optimiser that is not in
        `parameters` is stepped with its gradient unscaled, a tensor of `parameters` alone is scaled only.
      step: False clips only; no state is created and no step is counted.
      workspace: an optional uint8 device tensor of workspace_bytes(optimizer, parameters) to reuse between calls.
    Only tensors that have a gradient take part, as in torch. Missing state is created as torch creates it (exp_avg and exp_avg_sq zeros_like, `step` the
    CPU float32 torch.tensor(0.) of a non-capturable, non-fused Adam) and `step` is incremented on the host. The arithmetic is the numeric contract of
    include/gmpe.h; the bits are a function of the shapes, the sets and the data. Nothing here waits for the device, and with a workspace nothing is
    allocated per call beyond the outputs."""
    clip = max_grad_norm is not None
    if clip:
        max_grad_norm = float(max_grad_norm)
        if not max_grad_norm > 0.0:
            raise ValueError("max_grad_norm must be positive (or None: the norm is only reported), not %r" % (max_grad_norm,))
    step = bool(step)
    hypers, rows, dev = _table(optimizer, parameters, step)
    if len(rows) > _lib.OPT_MAX_PLAN_TENSORS:
        raise ValueError("%d tensors with gradients: one call takes at most %d" % (len(rows), _lib.OPT_MAX_PLAN_TENSORS))
    if not rows:                                        # nothing has a gradient: clip_grad_norm_ of nothing
        return torch.zeros((), dtype=torch.float32, device=dev)
    n = len(rows)
    table = bytearray(n * _TENSOR.size)                 # gmpe_optim_tensor[n], one pack per tensor: field by field through ctypes costs several times that
    keys, steps = {}, []
    for i, (p, flags, gi, st) in enumerate(rows):
        if st is None:
            _TENSOR.pack_into(table, i * _TENSOR.size, 0, p.grad.data_ptr(), 0, 0, p.numel(), flags, 0)
            continue
        if not st:
            _new_state(st, p)
        t = st["step"]
        steps.append(t)
        _TENSOR.pack_into(table, i * _TENSOR.size, p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel(), flags,
                          keys.setdefault((gi, int(t) + 1), len(keys)))
    tensors = C.cast((C.c_char * len(table)).from_buffer(table), C.POINTER(_lib.GmpeOptimTensor))
    hyper = (_lib.GmpeOptimHyper * max(len(keys), 1))()
    for (gi, t), k in keys.items():
        h = hyper[k]
        h.lr, h.beta1, h.beta2, h.eps, h.weight_decay = hypers[gi]
        h.t = t
    plan = _lib.GmpeOptimPlan()
    plan.n_tensors, plan.n_hypers, plan.tensors, plan.hypers = n, len(keys), tensors, hyper
    plan.flags = (_lib.OPT_CLIP if clip else 0) | (_lib.OPT_STEP if step else 0)
    plan.max_norm = max_grad_norm if clip else 0.0
    lib = _lib.load()
    need = C.c_size_t()
    _lib.check(lib.gmpe_optim_workspace_bytes(C.byref(plan), C.byref(need)), "gmpe_optim_workspace_bytes")
    workspace = _workspace(int(need.value), workspace, dev)
    out = torch.empty((2,), dtype=torch.float64, device=dev)
    grad_norm = torch.empty((), dtype=torch.float32, device=dev)
    plan.out, plan.grad_norm_f32 = out.data_ptr(), grad_norm.data_ptr()
    plan.workspace, plan.workspace_bytes = workspace.data_ptr(), workspace.numel()
    _lib.check(lib.gmpe_optim_step(_ordinal(dev), C.byref(plan), _stream_of(dev)), "gmpe_optim_step")
    if steps and all(isinstance(t, torch.Tensor) for t in steps):
        torch._foreach_add_(steps, 1)                   # torch's own way over its host-side step counts: one call
    else:
        for _, _, _, st in rows:
            if st is not None:
                st["step"] += 1
    return grad_norm
