"""The gradient clip and the Adam step of GR_MAPPO.ppo_update on the device (include/gmpe.h gmpe_optim_step): nn.utils.clip_grad_norm_ followed by
torch.optim.Adam.step (onpolicy/algorithms/graph_mappo.py:212-227, :254-265) as two launches per 64 tensors, with nothing that waits for the device.

    grad_norm = gmpe.clip_and_step(optimizer, max_grad_norm, parameters=net.parameters())
    # was: grad_norm = nn.utils.clip_grad_norm_(net.parameters(), max_grad_norm); optimizer.step()

For a data-parallel learner (include/gmpe.h gmpe_optim_step_shard) the same call with shards=x works on the sum over the ranks of their gradients, taken in
rank order in double and rounded once — clip_and_step_begin, x.exchange(.local), clip_and_step_finish: one launch per 64 tensors before the all-gather
and two after it. No DistributedDataParallel is involved, and the replicas stay bit-identical.

For a captured graph of the step (include/gmpe.h gmpe_optim_step_scheduled) ScheduledStep is the same call over a table built once, with Adam's step count
in device memory: .step() has the same kernel arguments at every call, so torch.cuda.graph can replay it; gmpe.policy.CapturedUpdate replays a whole
ppo_update on it.

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
_TENSOR = struct.Struct("@PPPPqii")                 # gmpe_optim_tensor; tests/test_optim_host.py holds its size, tests/test_abi_host.py _lib's layout to the header
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


def _max_norm(max_grad_norm):
    """-> (clip, max_grad_norm as a float)"""
    if max_grad_norm is None:
        return False, 0.0
    max_grad_norm = float(max_grad_norm)
    if not max_grad_norm > 0.0:
        raise ValueError("max_grad_norm must be positive (or None: the norm is only reported), not %r" % (max_grad_norm,))
    return True, max_grad_norm


_NO_GROUP = (0.0, 0.0, 0.0, 1.0, 0.0)                # the hyper-parameters of a table that steps nothing but carries `extra`: any valid set will do


def _bind(hypers, rows, clip, max_grad_norm, step, create=True, carry=None):
    """The gmpe_optim_plan over _table's rows, without outputs and workspace -> (plan, what it points to, the states' step counts).
    create False (clip_and_step_begin): missing state is not created — such a tensor has null pointers and the step count 1 it will have.
    carry: (total [k], scratch [3k]) of clip_and_step_begin's `extra`, the table's last tensor: stepped only, so that it is packed and summed like a
    gradient and never scaled; its parameter and its state are scratch."""
    n = len(rows) + (carry is not None)
    table = bytearray(n * _TENSOR.size)                 # gmpe_optim_tensor[n], one pack per tensor: field by field through ctypes costs several times that
    keys, steps = {}, []
    for i, (p, flags, gi, st) in enumerate(rows):
        if st is None:
            _TENSOR.pack_into(table, i * _TENSOR.size, 0, p.grad.data_ptr(), 0, 0, p.numel(), flags, 0)
            continue
        if not st:
            if not create:
                _TENSOR.pack_into(table, i * _TENSOR.size, 0, p.grad.data_ptr(), 0, 0, p.numel(), flags, keys.setdefault((gi, 1), len(keys)))
                continue
            _new_state(st, p)
        t = st["step"]
        steps.append(t)
        _TENSOR.pack_into(table, i * _TENSOR.size, p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel(), flags,
                          keys.setdefault((gi, int(t) + 1), len(keys)))
    if carry is not None:
        total, scratch = carry
        k, s = total.numel(), scratch.data_ptr()
        if not keys:
            keys[(None, 1)] = 0
        _TENSOR.pack_into(table, (n - 1) * _TENSOR.size, s, total.data_ptr(), s + 4 * k, s + 8 * k, k, _lib.OPT_T_STEP, 0)
    tensors = C.cast((C.c_char * len(table)).from_buffer(table), C.POINTER(_lib.GmpeOptimTensor))
    hyper = (_lib.GmpeOptimHyper * max(len(keys), 1))()
    for (gi, t), k in keys.items():
        h = hyper[k]
        h.lr, h.beta1, h.beta2, h.eps, h.weight_decay = _NO_GROUP if gi is None else hypers[gi]
        h.t = t
    plan = _lib.GmpeOptimPlan()
    plan.n_tensors, plan.n_hypers, plan.tensors, plan.hypers = n, len(keys), tensors, hyper
    plan.flags = (_lib.OPT_CLIP if clip else 0) | (_lib.OPT_STEP if step else 0)
    plan.max_norm = max_grad_norm if clip else 0.0
    return plan, (table, tensors, hyper), steps


def _outputs(plan, workspace, dev):
    """the plan's outputs and workspace -> (grad_norm, what the plan points to)"""
    out = torch.empty((2,), dtype=torch.float64, device=dev)
    grad_norm = torch.empty((), dtype=torch.float32, device=dev)
    plan.out, plan.grad_norm_f32 = out.data_ptr(), grad_norm.data_ptr()
    plan.workspace, plan.workspace_bytes = workspace.data_ptr(), workspace.numel()
    return grad_norm, out


def _count(steps, rows):
    if steps and all(isinstance(t, torch.Tensor) for t in steps):
        torch._foreach_add_(steps, 1)                   # torch's own way over its host-side step counts: one call
    else:
        for _, _, _, st in rows:
            if st is not None:
                st["step"] += 1


def _too_many(n):
    if n > _lib.OPT_MAX_PLAN_TENSORS:
        raise ValueError("%d tensors with gradients: one call takes at most %d" % (n, _lib.OPT_MAX_PLAN_TENSORS))


@torch.no_grad()
def clip_and_step(optimizer, max_grad_norm=None, *, parameters=None, step=True, workspace=None, shards=None, extra=None):
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
      shards: None, or the exchange of a data-parallel learner (gmpe.learner_shards): the gradients are this rank's contribution — the backward of
        ppo_losses(..., shards=shards, reduce="sum") — and the clip and the step work on the SUM over the ranks: clip_and_step_begin,
        shards.exchange(.local), clip_and_step_finish, which see. extra (with shards only): clip_and_step_begin's; the call then returns
        (grad_norm, extra_sum).
    Only tensors that have a gradient take part, as in torch. Missing state is created as torch creates it (exp_avg and exp_avg_sq zeros_like, `step` the
    CPU float32 torch.tensor(0.) of a non-capturable, non-fused Adam) and `step` is incremented on the host. The arithmetic is the numeric contract of
    include/gmpe.h; the bits are a function of the shapes, the sets and the data. Nothing here waits for the device, and with a workspace nothing is
    allocated per call beyond the outputs."""
    if shards is not None:
        from . import learner_shards
        world = learner_shards.check_shards(shards)
        h = clip_and_step_begin(optimizer, max_grad_norm, parameters=parameters, step=step, workspace=workspace, extra=extra)
        if h.local.numel() == 0:                        # no tensor has a gradient, on any rank: nothing is exchanged
            return clip_and_step_finish(h, h.local.new_empty((world, 0)))
        return clip_and_step_finish(h, learner_shards.gather(shards, h.local, "clip_and_step", torch.float32))
    if extra is not None:
        raise ValueError("extra rides on the exchange of shards: without shards there is none")
    clip, max_grad_norm = _max_norm(max_grad_norm)
    step = bool(step)
    hypers, rows, dev = _table(optimizer, parameters, step)
    _too_many(len(rows))
    if not rows:                                        # nothing has a gradient: clip_grad_norm_ of nothing
        return torch.zeros((), dtype=torch.float32, device=dev)
    plan, keep, steps = _bind(hypers, rows, clip, max_grad_norm, step)
    lib = _lib.load()
    need = C.c_size_t()
    _lib.check(lib.gmpe_optim_workspace_bytes(C.byref(plan), C.byref(need)), "gmpe_optim_workspace_bytes")
    grad_norm, out = _outputs(plan, _workspace(int(need.value), workspace, dev), dev)
    _lib.check(lib.gmpe_optim_step(_ordinal(dev), C.byref(plan), _stream_of(dev)), "gmpe_optim_step")
    _count(steps, rows)
    return grad_norm


STEPS_AHEAD = 1024


class _Budget(object):
    """The host's count of a schedule's rows: `issued` steps launched from the host, `advanced` steps the host-side step counts were moved by (a replayed
    graph launches nothing from here, so its steps are only ever advanced). The device counter stands at the larger of the two."""

    def __init__(self, rows):
        self.rows, self.issued, self.advanced = int(rows), 0, 0

    @property
    def remaining(self):
        return self.rows - max(self.issued, self.advanced)

    def need(self, fn, n=1):
        if self.remaining < n:
            raise RuntimeError("%s: the schedule holds %d steps and %d are used: %d more would run past it (refill() first, or build it with a larger "
                               "steps_ahead)" % (fn, self.rows, self.rows - self.remaining, n))


class ScheduledStep(object):
    """clip_and_step over a table that is built once, with Adam's step count on the device (include/gmpe.h gmpe_optim_step_scheduled): the float32
    hyper-parameter sets of the next `steps_ahead` step counts lie in device memory, a device counter picks the row and the call's last launch advances
    it. The kernel arguments are the same at every call, so .step() may be captured in a torch.cuda.graph and replayed; its bits are clip_and_step's.

        sched = gmpe.optim.ScheduledStep(optimizer, max_grad_norm, parameters=net.parameters())      # after a backward: the gradients exist
        grad_norm = sched.step(); sched.advance_host()                                                 # == clip_and_step(optimizer, max_grad_norm, ...)

      optimizer, max_grad_norm, parameters, workspace: clip_and_step's, with its refusals, all at construction. The table holds the tensors that have a
        gradient NOW; missing Adam state is created as torch creates it. The gradients must stay these tensors (write new values into them: backward
        into a kept .grad, or copy_): .step() raises RuntimeError when a .grad was replaced. shards= is not offered (no collective inside a graph).
      steps_ahead: rows of the schedule. .remaining counts the unused ones on the host; .step() raises RuntimeError instead of launching past the last
        (a raw C caller gets the device-side status, .status, set to 1 and nothing touched).
      .step() -> grad_norm, ONE static 0-dim float32 device tensor that every call overwrites. It does not move the host-side step counts:
      .advance_host(n) adds n to state["step"] of every stepped tensor — after n steps or replays optimizer.state_dict() is what n clip_and_step calls
        leave, and torch's step() or clip_and_step can take over.
      .refill() re-reads param_groups (a decayed lr) and the host step counts, rewrites the schedule and zeroes the counter with copies on the current
        stream, nothing waits. A graph captured before stays valid: the addresses do not change."""

    def __init__(self, optimizer, max_grad_norm=None, *, parameters=None, steps_ahead=STEPS_AHEAD, workspace=None):
        self.clip, self.max_grad_norm = _max_norm(max_grad_norm)
        steps_ahead = int(steps_ahead)
        if not 1 <= steps_ahead <= _lib.OPT_MAX_SCHEDULE_ROWS:
            raise ValueError("steps_ahead must be in 1 .. %d, not %d" % (_lib.OPT_MAX_SCHEDULE_ROWS, steps_ahead))
        self.optimizer = optimizer
        with torch.no_grad():
            hypers, rows, dev = _table(optimizer, parameters, True)
            _too_many(len(rows))
            if not rows:
                raise ValueError("no tensor has a gradient: ScheduledStep builds its table from the gradients there are (run a backward first)")
            self.rows, self.dev = rows, dev
            self.grads = [p.grad for p, _, _, _ in rows]
            self._bind(hypers)
            lib = _lib.load()
            need = C.c_size_t()
            _lib.check(lib.gmpe_optim_workspace_bytes(C.byref(self.plan.base), C.byref(need)), "gmpe_optim_workspace_bytes")
            self.workspace = _workspace(int(need.value), workspace, dev)
            self.grad_norm, self.out = _outputs(self.plan.base, self.workspace, dev)
            _lib.check(lib.gmpe_optim_schedule_bytes(C.byref(self.plan.base), steps_ahead, C.byref(need)), "gmpe_optim_schedule_bytes")
            self.schedule = torch.zeros((int(need.value) // 4,), dtype=torch.float32, device=dev)
            self.counter = torch.zeros((1,), dtype=torch.int32, device=dev)
            self.status = torch.zeros((1,), dtype=torch.int32, device=dev)
            self.plan.schedule, self.plan.counter, self.plan.status = self.schedule.data_ptr(), self.counter.data_ptr(), self.status.data_ptr()
            self.plan.rows = steps_ahead
            self._upload()

    def _bind(self, hypers):
        base, self._keep, self.steps = _bind(hypers, self.rows, self.clip, self.max_grad_norm, True)
        plan = getattr(self, "plan", None)
        if plan is None:
            self.plan = plan = _lib.GmpeOptimSchedPlan()
        else:                                               # refill: the table must be the one the schedule's slots were laid out for
            if bytes(self._keep[0]) != self._table_bytes:
                raise RuntimeError("the table changed (a parameter, its state or its step count no longer matches): build a new ScheduledStep")
            base.out, base.grad_norm_f32, base.workspace, base.workspace_bytes = plan.base.out, plan.base.grad_norm_f32, plan.base.workspace, \
                plan.base.workspace_bytes
        plan.base = base
        self._table_bytes, self.hypers = bytes(self._keep[0]), hypers

    def _upload(self):
        host = torch.empty((self.schedule.numel(),), dtype=torch.float32, pin_memory=True)
        _lib.check(_lib.load().gmpe_optim_schedule_fill(C.byref(self.plan.base), self.plan.rows, host.data_ptr()), "gmpe_optim_schedule_fill")
        self.schedule.copy_(host, non_blocking=True)
        self.counter.zero_()
        self._budget = _Budget(self.plan.rows)

    @property
    def remaining(self):
        return self._budget.remaining

    def check_grads(self):
        if any(p.grad is not g for (p, _, _, _), g in zip(self.rows, self.grads)):
            raise RuntimeError("a gradient was replaced since the ScheduledStep was built: its table holds the tensors that were .grad then "
                               "(write into them, e.g. zero_grad(set_to_none=False))")

    def stale(self):
        """whether param_groups no longer hold the hyper-parameters the schedule was filled with"""
        return _groups(self.optimizer) != self.hypers

    @torch.no_grad()
    def step(self):
        capturing = torch.cuda.is_current_stream_capturing()
        if not capturing:
            self._budget.need("ScheduledStep.step")
        self.check_grads()
        _lib.check(_lib.load().gmpe_optim_step_scheduled(_ordinal(self.dev), C.byref(self.plan), _stream_of(self.dev)), "gmpe_optim_step_scheduled")
        if not capturing:
            self._budget.issued += 1
        return self.grad_norm

    def advance_host(self, n=1):
        n = int(n)
        if n < 0:
            raise ValueError("n must be >= 0")
        if self.steps and all(isinstance(t, torch.Tensor) for t in self.steps):
            torch._foreach_add_(self.steps, n)
        else:
            for _, _, _, st in self.rows:
                if st is not None:
                    st["step"] += n
        self._budget.advanced += n

    @torch.no_grad()
    def refill(self):
        if self._budget.issued > self._budget.advanced:
            raise RuntimeError("ScheduledStep.refill: %d steps were issued and the host step counts advanced by %d: advance_host() first, the new "
                               "schedule starts at the host's counts" % (self._budget.issued, self._budget.advanced))
        self.check_grads()
        self._bind(_groups(self.optimizer))
        self._upload()


MAX_EXTRA = 16


class ClipAndStepShard(object):
    """What clip_and_step_begin leaves for clip_and_step_finish: `.local`, float32 [n + k] on the device (valid once the stream reaches it) — this rank's
    gradients packed back to back in table order, then the k elements of `extra` — and the call's table with the tensors it points to."""

    def __init__(self, optimizer, hypers, rows, dev, clip, max_grad_norm, step, carry, workspace, local):
        self.optimizer, self.hypers, self.rows, self.dev, self.clip, self.max_grad_norm, self.step = optimizer, hypers, rows, dev, clip, max_grad_norm, step
        self.carry, self.workspace, self.local, self.done = carry, workspace, local, False
        self.grads = [p.grad for p, _, _, _ in rows]    # the tensors LOCAL read: APPLY writes the sums to the same ones


def _shard_plan(plan, phase, world, local, all_, n):
    sp = _lib.GmpeOptimShardPlan()
    sp.base = plan
    sp.phase, sp.world, sp.local, sp.all, sp.local_elems = phase, world, local, all_, n
    return sp


@torch.no_grad()
def clip_and_step_begin(optimizer, max_grad_norm=None, *, parameters=None, step=True, workspace=None, extra=None):
    """The first phase of clip_and_step over one shard of a data-parallel learner (gmpe_optim_step_shard, GMPE_SHARD_LOCAL), same arguments: one launch
    per 64 tensors packs the gradients of every tensor of the call, clipped or stepped, into the handle's `.local`. Every refusal of clip_and_step
    happens here; no state is created, no step is counted and no gradient is changed. -> ClipAndStepShard
      extra: None, or a float32 tensor of at most 16 elements on the gradients' device. It rides behind the gradients in `.local` and comes back from
        clip_and_step_finish as the sum over the ranks by the gradients' own rule — global scalars out of the collective that is paid for anyway.
    The tables of all ranks must be equal — the same tensors with gradients, in the same order — and so must `extra`'s length: what is exchanged is
    positions, not names. Between begin and finish the gradients must stay the tensors they are. A call in which no tensor has a gradient and no extra
    is given leaves an empty `.local`: there is nothing to exchange, provided all ranks are in that state together."""
    clip, max_grad_norm = _max_norm(max_grad_norm)
    step = bool(step)
    if extra is not None:
        if not isinstance(extra, torch.Tensor) or extra.dtype != torch.float32:
            raise ValueError("extra must be a float32 tensor")
        if extra.numel() > MAX_EXTRA:
            raise ValueError("extra must have at most %d elements, not %d" % (MAX_EXTRA, extra.numel()))
    hypers, rows, dev = _table(optimizer, parameters, step)
    _too_many(len(rows) + (extra is not None))
    carry = None
    if extra is not None:
        if extra.device != dev:
            raise ValueError("extra is on %s: it must be on %s (the device of the gradients)" % (extra.device, dev))
        k = extra.numel()
        carry = (extra.detach().reshape(-1).clone(), torch.zeros((3 * k,), dtype=torch.float32, device=dev))
    local = torch.empty((0,), dtype=torch.float32, device=dev)
    if rows or (carry is not None and carry[0].numel()):
        plan, keep, _ = _bind(hypers, rows, clip, max_grad_norm, step, create=False, carry=carry)
        lib = _lib.load()
        n, need = C.c_int64(), C.c_size_t()
        _lib.check(lib.gmpe_optim_shard_elems(C.byref(plan), C.byref(n)), "gmpe_optim_shard_elems")
        _lib.check(lib.gmpe_optim_workspace_bytes(C.byref(plan), C.byref(need)), "gmpe_optim_workspace_bytes")
        workspace = _workspace(int(need.value), workspace, dev)
        if n.value:
            local = torch.empty((n.value,), dtype=torch.float32, device=dev)
            sp = _shard_plan(plan, _lib.SHARD_LOCAL, 1, local.data_ptr(), None, n.value)
            _lib.check(lib.gmpe_optim_step_shard(_ordinal(dev), C.byref(sp), _stream_of(dev)), "gmpe_optim_step_shard")
    return ClipAndStepShard(optimizer, hypers, rows, dev, clip, max_grad_norm, step, carry, workspace, local)


@torch.no_grad()
def clip_and_step_finish(handle, all):
    """The second phase (GMPE_SHARD_APPLY), two launches per 64 tensors: all float32 [world, n + k], contiguous, on the handle's device, row r = rank r's
    `.local` (torch.stack in one process, an all-gather across ranks). Every element becomes the sum of its column in rank order, in double, rounded
    once — a sum, not a mean: the ranks' gradients of ppo_losses(..., reduce="sum") add up to the whole minibatch's. The sums are written to the
    gradients (p.grad holds the global gradient afterwards, as under DDP), then clip_and_step's norm, clip and Adam step run on them; state is created
    and `step` counted here. Every rank computes the same bits from the same rows, so the replicas' parameters, Adam state and norm stay bit-identical.
    `all` is checked before any launch (a wrong row length — unequal tables — is caught here). Once per handle.
    -> grad_norm, or (grad_norm, extra_sum [k]) when begin was given `extra`."""
    from . import learner_shards
    if not isinstance(handle, ClipAndStepShard):
        raise TypeError("handle must come from clip_and_step_begin")
    if handle.done:
        raise RuntimeError("clip_and_step_finish was already called on this handle (it would step twice)")
    h, dev = handle, handle.dev
    world = learner_shards.check_all_stats(all, h.local, "clip_and_step_finish", torch.float32)
    if any(p.grad is not g for (p, _, _, _), g in zip(h.rows, h.grads)):
        raise RuntimeError("a gradient was replaced between clip_and_step_begin and clip_and_step_finish")
    n = int(h.local.numel())
    if n == 0:
        grad_norm = torch.zeros((), dtype=torch.float32, device=dev)
    else:
        plan, keep, steps = _bind(h.hypers, h.rows, h.clip, h.max_grad_norm, h.step, carry=h.carry)
        grad_norm, out = _outputs(plan, h.workspace, dev)
        sp = _shard_plan(plan, _lib.SHARD_APPLY, world, None, all.data_ptr(), n)
        _lib.check(_lib.load().gmpe_optim_step_shard(_ordinal(dev), C.byref(sp), _stream_of(dev)), "gmpe_optim_step_shard")
        _count(steps, h.rows)
    h.done = True
    return grad_norm if h.carry is None else (grad_norm, h.carry[0])
