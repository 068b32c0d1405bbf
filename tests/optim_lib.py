"""What the tests of gmpe.clip_and_step share (include/gmpe.h gmpe_optim_step): the clip and the Adam step restated in float64 numpy, the parameter sets
and their gradients, torch's own run of the same steps on the CPU, the restated launch geometry, and the error metric.

The metric is relative to the array's own size, err(a, t) = max|a - t| / max|t|: exp_avg_sq lies far below 1, where the max(1, .) form of the other
suites would hide any error. The rule is the project's: err_dev <= 4 * err_ref + 2^-23 with err_ref <= 1e-5, err_ref from torch's float32
run on the CPU against the float64 restatement."""
import numpy as np
import torch

CHUNK, MAX_TENSORS, MAX_HYPERS = 1024, 64, 8            # GMPE_OPT_CHUNK, GMPE_OPT_MAX_TENSORS, GMPE_OPT_MAX_HYPERS
GROUP_LIMIT = 0x7fffffff - CHUNK
IN_NORM, STEP = 1, 2
CAP, FLOOR = 1e-5, 2.0 ** -23
ARRAYS = ("param", "grad", "exp_avg", "exp_avg_sq")
SHAPES = ((1,), (16,), (16, 9), (48, 16), (192, 64), (3, 7), (CHUNK - 1,), (CHUNK,), (CHUNK + 1,), (2 * CHUNK + 3,))
STEPS, LR, EPS, MAX_NORM = 5, 1e-2, 1e-5, 100.0


def err(a, t):
    a, t = np.asarray(a, np.float64).reshape(-1), np.asarray(t, np.float64).reshape(-1)
    assert a.shape == t.shape
    if a.size == 0:
        return 0.0
    d, size = float(np.abs(a - t).max()), float(np.abs(t).max())
    return d / size if size > 0 else d


def bound(err_ref):
    return 4.0 * err_ref + FLOOR


def parameters(shapes, seed=0):
    """float32 arrays, one per shape"""
    rng = np.random.RandomState(seed)
    return [rng.randn(*s).astype(np.float32) for s in shapes]


def gradients(shapes, step, seed=0):
    """tensor i: randn * 10^(i mod 4 - 2), times 3 at the first step and 0.05 afterwards"""
    rng = np.random.RandomState(1000 * (seed + 1) + step)
    scale = 3.0 if step == 0 else 0.05
    return [(rng.randn(*s) * 10.0 ** (i % 4 - 2) * scale).astype(np.float32) for i, s in enumerate(shapes)]


class Restated(object):
    """clip_grad_norm_ + Adam.step in plain float64, tensor by tensor; state and step counts per tensor, created at a tensor's first step as torch does"""

    def __init__(self, params):
        self.p = [np.asarray(p, np.float64).copy() for p in params]
        self.m = [None] * len(self.p)
        self.v = [None] * len(self.p)
        self.t = [0] * len(self.p)

    def step(self, grads, max_norm, lr=LR, betas=(0.9, 0.999), eps=EPS, weight_decay=0.0, in_norm=None, stepped=None):
        """grads: per tensor an array or None; in_norm / stepped: per tensor booleans (default: all); lr, eps, weight_decay: numbers or per tensor lists.
        -> (total_norm, the gradients after the clip)"""
        n = len(self.p)
        per = lambda x: list(x) if isinstance(x, (list, tuple)) else [x] * n
        lr, eps, weight_decay = per(lr), per(eps), per(weight_decay)
        in_norm = [True] * n if in_norm is None else in_norm
        stepped = [True] * n if stepped is None else stepped
        g = [None if x is None else np.asarray(x, np.float64).copy() for x in grads]
        total = np.sqrt(sum(float((x * x).sum()) for x, f in zip(g, in_norm) if x is not None and f))
        if max_norm is not None:
            with np.errstate(invalid="ignore"):
                c = np.float64(max_norm) / (total + 1e-6)
                coef = c if np.isnan(c) else min(1.0, c)
                g = [x * coef if x is not None and f else x for x, f in zip(g, in_norm)]
        b1, b2 = betas
        for i in range(n):
            if g[i] is None or not stepped[i]:
                continue
            if self.m[i] is None:
                self.m[i], self.v[i] = np.zeros_like(self.p[i]), np.zeros_like(self.p[i])
            self.t[i] += 1
            x = g[i] + weight_decay[i] * self.p[i] if weight_decay[i] != 0 else g[i]
            self.m[i] = self.m[i] + (x - self.m[i]) * (1 - b1)
            self.v[i] = b2 * self.v[i] + (1 - b2) * x * x
            denom = np.sqrt(self.v[i]) / np.sqrt(1 - b2 ** self.t[i]) + eps[i]
            self.p[i] = self.p[i] - (lr[i] / (1 - b1 ** self.t[i])) * (self.m[i] / denom)
        return float(total), g


def torch_params(params, dtype=torch.float32, device="cpu"):
    return [torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(p)).clone().to(dtype).to(device)) for p in params]      # never the caller's memory


def set_grads(ps, grads):
    for p, g in zip(ps, grads):
        p.grad = None if g is None else torch.from_numpy(np.ascontiguousarray(g)).clone().to(p.dtype).to(p.device)


def torch_steps(params, shapes, steps, dtype, weight_decay, max_norm=MAX_NORM, seed=0):
    """torch's clip_grad_norm_ + Adam.step on the CPU in `dtype` over the accuracy case's gradients -> per step a dict of lists (float64 arrays) and the norm"""
    ps = torch_params(params, dtype)
    opt = torch.optim.Adam(ps, lr=LR, eps=EPS, weight_decay=weight_decay)
    out = []
    for k in range(steps):
        set_grads(ps, gradients(shapes, k, seed))
        norm = torch.nn.utils.clip_grad_norm_(ps, max_norm)
        opt.step()
        out.append(snapshot(ps, opt, norm))
    return out


def snapshot(ps, opt, norm):
    f = lambda t: t.detach().double().cpu().numpy().copy()
    return {"param": [f(p) for p in ps], "grad": [f(p.grad) for p in ps], "exp_avg": [f(opt.state[p]["exp_avg"]) for p in ps],
            "exp_avg_sq": [f(opt.state[p]["exp_avg_sq"]) for p in ps], "norm": float(norm)}


def restated_steps(params, shapes, steps, weight_decay, max_norm=MAX_NORM, seed=0):
    r = Restated(params)
    out = []
    for k in range(steps):
        norm, g = r.step(gradients(shapes, k, seed), max_norm, weight_decay=weight_decay)
        out.append({"param": [x.copy() for x in r.p], "grad": g, "exp_avg": [x.copy() for x in r.m], "exp_avg_sq": [x.copy() for x in r.v], "norm": norm})
    return out


def errors(run, truth):
    """per array the largest err over the tensors, and the norm's"""
    e = {k: max(err(a, t) for a, t in zip(run[k], truth[k])) for k in ARRAYS}
    e["norm"] = abs(run["norm"] - truth["norm"]) / truth["norm"] if truth["norm"] > 0 else abs(run["norm"])
    return e


def geometry(tensors):
    """The launch groups of include/gmpe.h restated. tensors: [(numel, flags, hyper)] in table order -> [(tensors, elements, chunks)] per group, at least
    one group."""
    groups, cur, total, slots = [], 0, 0, []
    for numel, flags, hyper in tensors:
        if numel == 0:
            continue
        steps = bool(flags & STEP)
        new_slot = steps and hyper not in slots
        if cur == MAX_TENSORS or (new_slot and len(slots) == MAX_HYPERS) or total + numel > GROUP_LIMIT:
            groups.append((cur, total))
            cur, total, slots = 0, 0, []
            new_slot = steps
        if new_slot:
            slots.append(hyper)
        cur, total = cur + 1, total + numel
    groups.append((cur, total))
    return [(n, t, (t + CHUNK - 1) // CHUNK) for n, t in groups]


def workspace_bytes(tensors):
    return 8 * sum(c for _, _, c in geometry(tensors))
