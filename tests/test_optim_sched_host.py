"""Host side of the scheduled optimiser step (include/gmpe.h gmpe_optim_schedule_bytes / _fill / gmpe_optim_step_scheduled, gmpe.optim.ScheduledStep,
gmpe.policy.CapturedUpdate), no GPU:
(a) the schedule's rows are, bit for bit, the float32 sets gmpe_optim_step forms on the host for the step counts t, t + 1, ...: Python's float ** is the
    C library's pow, the one the library calls, and numpy rounds a double to float32 once, as the cast does;
(b) the slot layout the header states: n_groups * 8 slots of 7 floats per row, a group's slots in the order its stepped tensors first name a set;
(c) every refusal of the C entry and of the two Python objects happens on the host: where there is no device, a call that got past its arguments
    would fail with a HIP error instead of GMPE_ERR_INVALID_ARG."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

import gmpe
from gmpe import _lib, optim, policy
from test_optim_host import _plan

HF, MAXH, MAXT = _lib.OPT_HYPER_FLOATS, _lib.OPT_MAX_HYPERS, _lib.OPT_MAX_TENSORS
INVALID = -1


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).reshape(-1).view(np.uint32)


def want_set(h, t):
    """gmpe_optim_step's seven floats of one param_group at step count t, in the slot's order: wd, w1, b2, w2, a, s2, eps"""
    lr, b1, b2, eps, wd = h
    return np.array([np.float32(wd), np.float32(1.0 - b1), np.float32(b2), np.float32(1.0 - b2), np.float32(lr / (1.0 - b1 ** t)),
                     np.float32(math.sqrt(1.0 - b2 ** t)), np.float32(eps)], np.float32)


def filled(plan, rows):
    lib = _lib.load()
    n = C.c_size_t()
    assert lib.gmpe_optim_schedule_bytes(C.byref(plan), rows, C.byref(n)) == 0, lib.gmpe_last_error()
    buf = np.full((n.value // 4,), np.nan, np.float32)
    assert lib.gmpe_optim_schedule_fill(C.byref(plan), rows, buf.ctypes.data) == 0, lib.gmpe_last_error()
    return buf.reshape(rows, -1)


GROUPS = ((1e-3, 0.9, 0.999, 1e-8, 0.0), (7e-4, 0.8, 0.99, 1e-5, 1e-2))      # two param_groups: lr, beta1, beta2, eps, weight_decay all differ


def test_rows_are_the_sets_of_the_next_step_counts_bit_for_bit():
    sets = [GROUPS[0] + (1,), GROUPS[0] + (5,), GROUPS[1] + (1,), GROUPS[1] + (5,)]
    plan = _plan([(3, 3, 0), (1025, 3, 1), (3, 1, 0), (7, 3, 2), (5, 3, 3), (2, 3, 1)], sets=sets)
    rows = 6
    s = filled(plan, rows)
    assert s.shape == (rows, 1 * MAXH * HF)                                  # one launch group
    for k in range(rows):
        for slot, h in enumerate(sets):
            got, want = s[k, slot * HF:(slot + 1) * HF], want_set(h[:5], h[5] + k)
            assert np.array_equal(bits(got), bits(want)), (k, slot, got, want)
        assert not s[k, len(sets) * HF:].any()                               # slots not in use are 0
    # row 0 is what gmpe_optim_step itself uses: the bias corrections of t, and they move with k
    assert s[0, 4] != s[1, 4] and s[0, 5] != s[1, 5] and s[0, 4] == np.float32(1e-3 / (1.0 - 0.9))
    assert np.array_equal(s[4, 0:HF], s[0, HF:2 * HF])                       # group 0 at t = 1 + 4 is group 0 at t = 5 + 0


def test_slots_follow_the_launch_groups():
    lib = _lib.load()
    n = C.c_size_t()
    # 65 tensors: the 65th opens a second group, whose slot 0 is its own set
    sets = [GROUPS[0] + (1,), GROUPS[1] + (3,)]
    plan = _plan([(3, 3, 0)] * MAXT + [(3, 3, 1)], sets=sets)
    assert lib.gmpe_optim_schedule_bytes(C.byref(plan), 3, C.byref(n)) == 0 and n.value == 3 * 2 * MAXH * HF * 4
    s = filled(plan, 3)
    for k in range(3):
        assert np.array_equal(bits(s[k, 0:HF]), bits(want_set(GROUPS[0], 1 + k)))
        assert np.array_equal(bits(s[k, MAXH * HF:MAXH * HF + HF]), bits(want_set(GROUPS[1], 3 + k)))
        assert not s[k, HF:MAXH * HF].any() and not s[k, MAXH * HF + HF:].any()
    # nine distinct (group, t) keys: the ninth does not fit the first group's eight slots; the second group names sets 8 and then 2
    sets = [GROUPS[i % 2] + (1 + i,) for i in range(9)]
    plan = _plan([(3, 3, i) for i in range(9)] + [(3, 1, 0), (4, 3, 2)], sets=sets)
    s = filled(plan, 2)
    assert s.shape == (2, 2 * MAXH * HF)
    for k in range(2):
        for i in range(8):
            assert np.array_equal(bits(s[k, i * HF:(i + 1) * HF]), bits(want_set(GROUPS[i % 2], 1 + i + k))), (k, i)
        g1 = s[k, MAXH * HF:]
        assert np.array_equal(bits(g1[0:HF]), bits(want_set(GROUPS[0], 9 + k))) and np.array_equal(bits(g1[HF:2 * HF]), bits(want_set(GROUPS[0], 3 + k)))
        assert not g1[2 * HF:].any()
    # norm-only tensors take no slot; a table that steps nothing still has its one group's row
    plan = _plan([(3, 1, 0)] * 3, sets=[GROUPS[0] + (1,)])
    assert filled(plan, 2).shape == (2, MAXH * HF) and not filled(plan, 2).any()


def _sched(plan, rows=4, **over):
    sp = _lib.GmpeOptimSchedPlan()
    sp.base = plan
    sp.schedule, sp.counter, sp.status, sp.rows = 1 << 41, (1 << 41) + (1 << 30), (1 << 41) + (1 << 30) + 64, rows
    for k, v in over.items():
        setattr(sp, k, v)
    sp._keep = plan
    return sp


def test_the_c_entries_refuse_by_name_before_any_device_call():
    lib = _lib.load()
    table = [(3, 3, 0), (1025, 3, 0)]
    err = lambda: lib.gmpe_last_error().decode()
    cases = [
        (dict(rows=0), "rows must be in 1 .."),
        (dict(rows=_lib.OPT_MAX_SCHEDULE_ROWS + 1), "rows must be in 1 .."),
        (dict(reserved=1), "reserved must be 0"),
        (dict(schedule=None), "schedule is required with GMPE_OPT_STEP"),
        (dict(schedule=(1 << 41) + 2), "schedule must be 4-byte aligned"),
        (dict(counter=None), "counter is required"),
        (dict(counter=(1 << 41) + 1), "counter must be 4-byte aligned"),
        (dict(status=None), "status is required"),
        (dict(status=(1 << 41) + 3), "status must be 4-byte aligned"),
    ]
    for over, text in cases:
        rc = lib.gmpe_optim_step_scheduled(0, C.byref(_sched(_plan(table), **over)), None)
        assert rc == INVALID and "gmpe_optim_step_scheduled" in err() and text in err(), (over, rc, err())
    # base's own refusals, under this entry's name
    for over, text in [(dict(out=None), "out is required"), (dict(workspace=None), "workspace is required"), (dict(flags=4), "flags must be"),
                       (dict(max_norm=0.0), "max_norm must be > 0"), (dict(n_tensors=0), "n_tensors must be in")]:
        rc = lib.gmpe_optim_step_scheduled(0, C.byref(_sched(_plan(table, **over))), None)
        assert rc == INVALID and "gmpe_optim_step_scheduled" in err() and text in err(), (over, rc, err())
    rc = lib.gmpe_optim_step_scheduled(0, C.byref(_sched(_plan(table, sets=[GROUPS[0] + (0,)]))), None)
    assert rc == INVALID and "hypers[0].t must be >= 1" in err()
    assert lib.gmpe_optim_step_scheduled(0, None, None) == INVALID and "null plan" in err()
    # a clip-only plan needs no schedule, so it is refused for what comes next, not for that
    rc = lib.gmpe_optim_step_scheduled(0, C.byref(_sched(_plan(table, flags=1), schedule=None, counter=None)), None)
    assert rc == INVALID and "counter is required" in err()
    # the two host-only entries
    n = C.c_size_t()
    buf = np.zeros(4 * MAXH * HF, np.float32)
    assert lib.gmpe_optim_schedule_bytes(C.byref(_plan(table)), 4, None) == INVALID and "bytes_out is null" in err()
    assert lib.gmpe_optim_schedule_bytes(C.byref(_plan(table)), 0, C.byref(n)) == INVALID and "rows must be in" in err()
    assert lib.gmpe_optim_schedule_bytes(None, 4, C.byref(n)) == INVALID and "null plan" in err()
    assert lib.gmpe_optim_schedule_fill(C.byref(_plan(table)), 4, None) == INVALID and "host_dst is required" in err()
    assert lib.gmpe_optim_schedule_fill(C.byref(_plan(table)), -1, buf.ctypes.data) == INVALID and "rows must be in" in err()
    assert lib.gmpe_optim_schedule_fill(C.byref(_plan(table, sets=[(1e-3, 1.0, 0.999, 1e-8, 0.0, 1)])), 4, buf.ctypes.data) == INVALID \
        and "hypers[0].beta1 must be in [0, 1)" in err()
    assert lib.gmpe_optim_schedule_fill(C.byref(_plan([(3, 3, 1)])), 4, buf.ctypes.data) == INVALID and "hyper must index hypers" in err()
    # the geometry entries read no device pointer: a plan without outputs and workspace is enough for them
    bare = _plan(table, out=None, grad_norm_f32=None, workspace=None, workspace_bytes=0)
    assert lib.gmpe_optim_schedule_bytes(C.byref(bare), 4, C.byref(n)) == 0 and n.value == 4 * MAXH * HF * 4
    assert lib.gmpe_optim_schedule_fill(C.byref(bare), 4, buf.ctypes.data) == 0 and buf[4] == np.float32(1e-3 / (1.0 - 0.9))


def test_symbols_constants_and_the_struct():
    assert {"gmpe_optim_schedule_bytes", "gmpe_optim_schedule_fill", "gmpe_optim_step_scheduled"} <= set(_lib.SYMBOLS)
    assert (HF, _lib.OPT_MAX_SCHEDULE_ROWS) == (7, 1 << 20)
    assert C.sizeof(_lib.GmpeOptimSchedPlan) == C.sizeof(_lib.GmpeOptimPlan) + 32 and _lib.GmpeOptimSchedPlan.base.offset == 0
    assert callable(gmpe.optim.ScheduledStep) and callable(gmpe.policy.CapturedUpdate)


def _net():
    return torch.nn.Linear(3, 2)


def test_scheduled_step_refuses_on_the_host():
    net = _net()
    net(torch.ones(1, 3)).sum().backward()
    with pytest.raises(NotImplementedError, match="built for torch.optim.Adam"):
        optim.ScheduledStep(torch.optim.SGD(net.parameters(), lr=0.1), 1.0)
    with pytest.raises(NotImplementedError, match="amsgrad"):
        optim.ScheduledStep(torch.optim.Adam(net.parameters(), amsgrad=True), 1.0)
    adam = torch.optim.Adam(net.parameters())
    with pytest.raises(ValueError, match="max_grad_norm must be positive"):
        optim.ScheduledStep(adam, 0.0)
    with pytest.raises(ValueError, match="steps_ahead must be in 1"):
        optim.ScheduledStep(adam, 1.0, steps_ahead=0)
    with pytest.raises(ValueError, match="no CPU fallback"):                # CPU tensors: refused before anything is bound
        optim.ScheduledStep(adam, 1.0)
    assert not any(adam.state.values())                                      # no state was created on the way
    with pytest.raises(TypeError):
        optim.ScheduledStep(adam, 1.0, shards=object())                      # not offered


def test_a_step_past_the_schedule_is_refused_on_the_host():
    b = optim._Budget(3)
    assert b.remaining == 3
    for _ in range(3):
        b.need("ScheduledStep.step")
        b.issued += 1
        b.advanced += 1
    assert b.remaining == 0
    with pytest.raises(RuntimeError, match="ScheduledStep.step: the schedule holds 3 steps and 3 are used"):
        b.need("ScheduledStep.step")
    r = optim._Budget(5)                                                     # replays are only ever advanced
    r.advanced += 4
    assert r.remaining == 1
    r.need("CapturedUpdate.update")
    with pytest.raises(RuntimeError, match="CapturedUpdate.update"):
        r.need("CapturedUpdate.update", 2)


def test_captured_update_refuses_on_the_host():
    actor, critic = _net(), _net()
    adam = lambda n: torch.optim.Adam(n.parameters())
    sample = tuple(torch.zeros(4, 2) for _ in range(16))
    args = types.SimpleNamespace(use_popart=True)
    with pytest.raises(NotImplementedError, match="\"replace\" creates new Parameters"):
        policy.CapturedUpdate(actor, critic, adam(actor), adam(critic), sample, args, install="replace")
    with pytest.raises(NotImplementedError, match="built for torch.optim.Adam"):
        policy.CapturedUpdate(actor, critic, adam(actor), torch.optim.SGD(critic.parameters(), lr=0.1), sample, args)
    with pytest.raises(ValueError, match="value_head"):
        policy.CapturedUpdate(actor, critic, adam(actor), adam(critic), sample, args, value_head="host")
    with pytest.raises(ValueError, match="16-tuple"):
        policy.CapturedUpdate(actor, critic, adam(actor), adam(critic), sample[:15], args)
    with pytest.raises(ValueError, match="no CPU fallback"):
        policy.CapturedUpdate(actor, critic, adam(actor), adam(critic), sample, args)
    # a sample of another shape, dtype or make-up than the captured one
    static = tuple(None if i == 15 else torch.zeros(24, 2) for i in range(16))
    ok = tuple(None if i == 15 else torch.ones(24, 2) for i in range(16))
    policy._same_sample("CapturedUpdate.update", static, ok)
    other = list(ok)
    other[3] = torch.ones(48, 2)
    with pytest.raises(ValueError, match=r"sample\[3\] must be \(24, 2\)"):
        policy._same_sample("CapturedUpdate.update", static, tuple(other))
    other = list(ok)
    other[8] = torch.ones(24, 2, dtype=torch.int64)
    with pytest.raises(ValueError, match=r"sample\[8\] must be"):
        policy._same_sample("CapturedUpdate.update", static, tuple(other))
    other = list(ok)
    other[15] = torch.ones(24, 2)
    with pytest.raises(ValueError, match=r"sample\[15\] is given"):
        policy._same_sample("CapturedUpdate.update", static, tuple(other))
    with pytest.raises(ValueError, match="16-tuple"):
        policy._same_sample("CapturedUpdate.update", static, ok[:3])
