"""gmpe.optim.ScheduledStep (include/gmpe.h gmpe_optim_step_scheduled) on the device: the Adam step whose step count lives in device memory is, bit for
bit, gmpe.clip_and_step — called eagerly and as one captured graph replayed — and a call past its schedule touches nothing. One chunk is 1024 elements
per workgroup and a launch group holds 64 tensors and 8 hyper-parameter sets; the tables are the smallest that cross each of those edges. The eager
reference of a case is computed once and shared by the tests that compare with it."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import gmpe
from gmpe import _lib, optim

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEPS = 5
G0 = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
G1 = dict(lr=7e-4, betas=(0.8, 0.99), eps=1e-5, weight_decay=1e-2)
# case -> (sizes of the optimiser's tensors, the index where param_group 1 begins, the tensor that already has state at step 5 or None,
#          the optimiser's tensors left out of `parameters`, sizes of tensors that only `parameters` holds)
CASES = {
    "chunk-edges": ((1, 64, 1023, 1025, 2049), 3, 2, (), ()),           # 1, a wave, a chunk less one, a chunk and one, two chunks and one; two slots in group 0
    "two-launch-groups": ((3,) * 65, 40, 64, (), ()),                   # the 65th tensor opens a second launch group, with its own slot row
    "other-parameters": ((5, 1025, 7, 64), 2, None, (0,), (9, 1030)),   # tensor 0 is stepped unclipped (STEP only), two are clipped only (IN_NORM only)
}
NORMS = {"report": None, "clip": 1e-3, "no-clip": 1e9}


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


class Setup(object):
    """one optimiser over fresh tensors of a case; two of the same case are twins"""

    def __init__(self, case):
        sizes, cut, old, left_out, extra = CASES[case]
        g = torch.Generator().manual_seed(sum(sizes) + 7)
        self.ps = [torch.nn.Parameter((torch.rand(n, generator=g) * 2 - 1).to(DEV)) for n in sizes]
        self.extra = [torch.nn.Parameter((torch.rand(n, generator=g) * 2 - 1).to(DEV)) for n in extra]
        self.opt = torch.optim.Adam([dict(params=self.ps[:cut], **G0), dict(params=self.ps[cut:], **G1)])
        if old is not None:
            p = self.ps[old]
            self.opt.state[p] = {"step": torch.tensor(5.0), "exp_avg": (torch.rand(p.shape, generator=g) * 0.2 - 0.1).to(DEV),
                                 "exp_avg_sq": (torch.rand(p.shape, generator=g) * 0.01).to(DEV)}
        self.parameters = None if not (left_out or extra) else [p for i, p in enumerate(self.ps) if i not in left_out] + self.extra
        self.all = self.ps + self.extra
        self.case = case

    def write_grads(self, k):
        """step k's gradients, into the .grad tensors that are there (created at the first call)"""
        g = torch.Generator().manual_seed(1000 * k + len(self.all))
        for p in self.all:
            v = (torch.randn(p.shape, generator=g) * (0.5 + 0.1 * k)).to(DEV)
            if p.grad is None:
                p.grad = v
            else:
                p.grad.copy_(v)

    def snapshot(self, norm):
        out = {"norm": bits(norm)}
        for i, p in enumerate(self.all):
            st = self.opt.state.get(p, {})
            out[i] = (bits(p), bits(p.grad), bits(st["exp_avg"]) if st else None, bits(st["exp_avg_sq"]) if st else None)
        return out

    def state(self):
        sd = self.opt.state_dict()
        return {k: {n: (float(v) if n == "step" else bits(v)) for n, v in st.items()} for k, st in sd["state"].items()}, sd["param_groups"]


def equal_snapshots(a, b, what):
    assert sorted(map(str, a)) == sorted(map(str, b))
    assert np.array_equal(a["norm"], b["norm"]), (what, "norm")
    for k in a:
        if k != "norm":
            for name, x, y in zip(("param", "grad", "exp_avg", "exp_avg_sq"), a[k], b[k]):
                assert (x is None) == (y is None) and (x is None or np.array_equal(x, y)), (what, k, name)


def equal_states(a, b):
    (sa, ga), (sb, gb) = a, b
    assert ga == gb and sorted(sa) == sorted(sb)
    for k in sa:
        assert sorted(sa[k]) == sorted(sb[k])
        for n in sa[k]:
            assert sa[k][n] == sb[k][n] if n == "step" else np.array_equal(sa[k][n], sb[k][n]), (k, n)


@functools.lru_cache(maxsize=None)
def eager(case, norm):
    """STEPS eager clip_and_step calls -> (the snapshot after each, the final state_dict as state() gives it)"""
    s = Setup(case)
    snaps = []
    for k in range(STEPS):
        s.write_grads(k)
        snaps.append(s.snapshot(gmpe.clip_and_step(s.opt, NORMS[norm], parameters=s.parameters)))
    torch.cuda.synchronize()
    return snaps, s.state()


def scheduled(case, norm, **kw):
    s = Setup(case)
    s.write_grads(0)
    return s, optim.ScheduledStep(s.opt, NORMS[norm], parameters=s.parameters, **kw)


@pytest.mark.parametrize("norm", list(NORMS))
@pytest.mark.parametrize("case", list(CASES))
def test_five_steps_are_clip_and_steps_bit_for_bit(case, norm):
    want, want_state = eager(case, norm)
    s, sched = scheduled(case, norm, steps_ahead=STEPS)
    assert sched.remaining == STEPS
    for k in range(STEPS):
        if k:
            s.write_grads(k)
        n = sched.step()
        assert n is sched.grad_norm and n.dim() == 0 and n.dtype == torch.float32
        equal_snapshots(s.snapshot(n), want[k], "%s %s step %d" % (case, norm, k))
    assert sched.remaining == 0 and int(sched.counter) == STEPS and int(sched.status) == 0
    sched.advance_host(STEPS)
    equal_states(s.state(), want_state)
    # the optimiser is torch's own again: clip_and_step takes over from the counts advance_host left
    ref = Setup(case)
    for k in range(STEPS):
        ref.write_grads(k)
        gmpe.clip_and_step(ref.opt, NORMS[norm], parameters=ref.parameters)
    for x in (s, ref):
        x.write_grads(STEPS)
    a, b = gmpe.clip_and_step(s.opt, NORMS[norm], parameters=s.parameters), gmpe.clip_and_step(ref.opt, NORMS[norm], parameters=ref.parameters)
    equal_snapshots(s.snapshot(a), ref.snapshot(b), "after the hand-over")


@pytest.mark.parametrize("norm", list(NORMS))
@pytest.mark.parametrize("case", list(CASES))
def test_one_captured_step_replayed_five_times_gives_the_same_bits(case, norm):
    want, want_state = eager(case, norm)
    warm, wsched = scheduled(case, norm, steps_ahead=1)
    wsched.step()                                                            # every kernel of the call is loaded before anything is captured
    s, sched = scheduled(case, norm, steps_ahead=STEPS)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        n = sched.step()
    assert sched.remaining == STEPS and int(sched.counter) == 0              # a capture runs nothing
    for k in range(STEPS):
        if k:
            s.write_grads(k)
        graph.replay()
        sched.advance_host()
        equal_snapshots(s.snapshot(n), want[k], "%s %s replay %d" % (case, norm, k))
    assert sched.remaining == 0 and int(sched.counter) == STEPS and int(sched.status) == 0
    equal_states(s.state(), want_state)


@pytest.mark.parametrize("norm", ["report", "clip"])
def test_a_call_past_the_schedule_touches_nothing_and_says_so(norm):
    s, sched = scheduled("chunk-edges", norm, steps_ahead=3)
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda: lib.gmpe_optim_step_scheduled(0, C.byref(sched.plan), stream)
    for k in range(3):
        assert call() == 0
    assert int(sched.counter) == 3 and int(sched.status) == 0
    s.write_grads(3)
    before = s.snapshot(torch.zeros(()))
    want_norm = gmpe.clip_and_step(s.opt, None, parameters=s.parameters, step=False)          # reports the norm, changes nothing
    sched.grad_norm.fill_(-1.0)
    sched.out.fill_(-1.0)
    assert call() == 0                                                       # the device is the backstop of a raw C caller: no error code, a sticky flag
    after = s.snapshot(torch.zeros(()))
    equal_snapshots(before, after, "the fourth call")
    assert int(sched.status) == 1 and int(sched.counter) == 3
    assert same(sched.grad_norm, want_norm) and float(sched.out[0]) == pytest.approx(float(want_norm), rel=1e-6) and float(want_norm) > 1.0
    assert call() == 0 and int(sched.status) == 1 and int(sched.counter) == 3
    equal_snapshots(before, s.snapshot(torch.zeros(())), "the fifth call")
    # the Python object counts on the host and never issues that call
    s2, sched2 = scheduled("chunk-edges", norm, steps_ahead=3)
    for k in range(3):
        sched2.step()
        sched2.advance_host()
    kept = s2.snapshot(sched2.grad_norm)
    with pytest.raises(RuntimeError, match="the schedule holds 3 steps and 3 are used"):
        sched2.step()
    assert int(sched2.status) == 0 and int(sched2.counter) == 3
    equal_snapshots(kept, s2.snapshot(sched2.grad_norm), "the refused step")


def test_refill_reads_the_decayed_lr_and_the_host_counts():
    a = Setup("chunk-edges")
    b, sched = scheduled("chunk-edges", "clip", steps_ahead=4)
    for k in range(2):
        a.write_grads(k)
        if k:
            b.write_grads(k)
        gmpe.clip_and_step(a.opt, NORMS["clip"], parameters=a.parameters)
        sched.step()
        sched.advance_host()
    assert not sched.stale()
    for x in (a, b):
        for g in x.opt.param_groups:
            g["lr"] = g["lr"] / 2
    assert sched.stale()
    # without a refill the schedule still holds the old lr: that step would differ
    sched.refill()
    assert sched.remaining == 4 and int(sched.counter) == 0 and not sched.stale()
    for k in (2, 3):
        a.write_grads(k)
        b.write_grads(k)
        na = gmpe.clip_and_step(a.opt, NORMS["clip"], parameters=a.parameters)
        nb = sched.step()
        sched.advance_host()
        equal_snapshots(b.snapshot(nb), a.snapshot(na), "step %d after the refill" % k)
    equal_states(a.state(), b.state())
    old = Setup("chunk-edges")                                               # the same four steps with the lr never halved end elsewhere
    for k in range(4):
        old.write_grads(k)
        gmpe.clip_and_step(old.opt, NORMS["clip"], parameters=old.parameters)
    assert not same(old.ps[4], a.ps[4])
    # steps issued and not yet counted on the host: the new schedule would start at stale counts
    b.write_grads(4)
    sched.step()
    with pytest.raises(RuntimeError, match="advance_host"):
        sched.refill()


def test_a_replaced_gradient_is_refused():
    s, sched = scheduled("other-parameters", "clip")
    assert sched.remaining == optim.STEPS_AHEAD
    sched.step()
    s.ps[1].grad = s.ps[1].grad.clone()
    with pytest.raises(RuntimeError, match="a gradient was replaced"):
        sched.step()
    bare = Setup("other-parameters")
    with pytest.raises(ValueError, match="no tensor has a gradient"):
        optim.ScheduledStep(bare.opt, 1.0, parameters=bare.parameters)
