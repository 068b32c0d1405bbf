"""Host side of the sharded gradient clip and Adam step (include/gmpe.h gmpe_optim_shard_elems / gmpe_optim_step_shard, gmpe.clip_and_step_begin /
_finish, shards= of gmpe.clip_and_step, gmpe.policy.ppo_update and gmpe.policy.train), no GPU: the struct and the symbols against the header, every
refusal of both layers before any device call (where there is no device, a call that got that far fails with a HIP error instead), the length of `local`
against the restated geometry, the restated combination rule on rows that tell rank orders apart, and the compiler's scratch report of the new kernels."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import abi_lib
import gmpe
import optim_lib as OL
import optim_shards_lib as SL
from gmpe import _lib, learner_shards, policy
from test_optim_host import _adam, _plan

FIELDS = ["base", "phase", "world", "local", "all", "local_elems"]


def test_the_shard_plan_matches_the_header_and_the_symbols_are_exported():
    PP = _lib.GmpeOptimShardPlan
    assert [f for f, _ in PP._fields_] == FIELDS
    assert abi_lib.layout(PP) == abi_lib.mirror_layout(PP)
    assert abi_lib.layout(PP)[0] == C.sizeof(_lib.GmpeOptimPlan) + 4 + 4 + 8 + 8 + 8 and abi_lib.layout(_lib.GmpeOptimPlan)[0] == C.sizeof(_lib.GmpeOptimPlan)
    assert [abi_lib.constant("GMPE_" + k) for k in ("SHARD_LOCAL", "SHARD_APPLY", "SHARD_MAX_WORLD", "ABI_VERSION")] == [
        _lib.SHARD_LOCAL, _lib.SHARD_APPLY, _lib.SHARD_MAX_WORLD, 3] == [0, 1, 4096, 3]
    assert {"gmpe_optim_shard_elems", "gmpe_optim_step_shard"} <= set(_lib.SYMBOLS) & abi_lib.exported()
    assert _lib.load().gmpe_abi_version() == 3 and gmpe.config.ABI_VERSION == 3          # added entry points: the ABI version stays
    assert gmpe.clip_and_step_begin is gmpe.optim.clip_and_step_begin and gmpe.clip_and_step_finish is gmpe.optim.clip_and_step_finish
    assert gmpe.optim.MAX_EXTRA == SL.MAX_EXTRA == 16


TWO = [(OL.CHUNK + 1, 3, 0), (7, 3, 0)]                 # 1032 elements: two chunks


def _shard_plan(table=TWO, phase=0, world=2, local=0x10000, all=0x20000, local_elems=None, **base):
    sp = _lib.GmpeOptimShardPlan()
    b = _plan(table, **base)
    sp.base = b
    sp.phase, sp.world, sp.local, sp.all = phase, world, local, all
    sp.local_elems = SL.elems([t if isinstance(t, tuple) else (t["numel"], 0, 0) for t in table]) if local_elems is None else local_elems
    sp._keep = b
    return sp


OWN_REFUSALS = [
    (dict(phase=2), "phase"), (dict(phase=-1), "phase"), (dict(world=0), "world"), (dict(world=4097), "world"), (dict(world=-3), "world"),
    (dict(phase=0, local=None), "local is required"), (dict(phase=0, local=0x10002), "local is required"), (dict(phase=1, all=None), "all is required"),
    (dict(phase=1, all=0x20001), "all is required"), (dict(local_elems=1031), "local_elems must be gmpe_optim_shard_elems(&base) = 1032"),
    (dict(phase=1, local_elems=0), "local_elems"), (dict(table=[(1 << 30, 1, 0)], world=2), "world * local_elems"),
    (dict(table=[(1 << 30, 1, 0)] * 2, world=1, phase=1, workspace_bytes=1 << 40), "world * local_elems"),
]
BASE_REFUSALS = [
    (dict(n_tensors=0), "n_tensors"), (dict(tensors=None), "tensors is null"), (dict(table=[(5, 0, 0)]), "tensors[0].flags"),
    (dict(table=[dict(numel=5, flags=3, hyper=0, grad=None)]), "tensors[0].grad is required"),
    (dict(table=[dict(numel=5, flags=3, hyper=0, grad=(1 << 20) + 1)]), "tensors[0].grad must be 4-byte"),
    # what only GMPE_SHARD_APPLY reads is asked for there, in gmpe_optim_step's words
    (dict(phase=1, out=None), "out is required"), (dict(phase=1, flags=4), "flags"), (dict(phase=1, max_norm=0.0), "max_norm"),
    (dict(phase=1, workspace=None), "workspace is required"), (dict(phase=1, workspace_bytes=8), "workspace_bytes is below gmpe_optim_workspace_bytes(plan) = 16"),
    (dict(phase=1, table=[dict(numel=5, flags=3, hyper=0, exp_avg=None)]), "tensors[0].exp_avg is required"),
    (dict(phase=1, sets=((-1e-3, 0.9, 0.999, 1e-8, 0.0, 1),)), "hypers[0].lr"),
]


def test_the_c_entry_refuses_by_name_before_any_device_call():
    lib = _lib.load()
    refused = lambda sp: (lib.gmpe_optim_step_shard(0, C.byref(sp) if sp is not None else None, None), lib.gmpe_last_error().decode())
    rc, msg = refused(None)
    assert rc == -1 and msg == "gmpe_optim_step_shard: null plan"
    for over, field in OWN_REFUSALS + BASE_REFUSALS:
        rc, msg = refused(_shard_plan(**over))
        assert rc == -1 and msg.startswith("gmpe_optim_step_shard: ") and field in msg, (over, msg)
    # its own fields are judged before the base plan's
    rc, msg = refused(_shard_plan(world=0, n_tensors=0))
    assert rc == -1 and "world" in msg
    # GMPE_SHARD_LOCAL reads the geometry and the gradients: a plan without parameters, state, hyper-parameter values, outputs or workspace passes every
    # check and, where there is no device, fails only at the device; so does a complete GMPE_SHARD_APPLY
    if not torch.cuda.is_available():
        bare = dict(numel=5, flags=3, hyper=0, param=None, exp_avg=None, exp_avg_sq=None)
        for sp in (_shard_plan([bare], out=None, grad_norm_f32=None, workspace=None, workspace_bytes=0, max_norm=-1.0, sets=((-1.0, 2.0, 2.0, -1.0, -1.0, 0),)),
                   _shard_plan(phase=1), _shard_plan(phase=1, world=4096), _shard_plan(phase=0, all=None), _shard_plan(phase=1, local=None)):
            rc, msg = refused(sp)
            assert rc != 0 and msg.startswith("hip"), msg


def test_shard_elems_is_the_restated_length_of_local():
    lib = _lib.load()
    n = C.c_int64(-1)
    cases = {
        "one element": [(1, 3, 0)],
        "the test shapes": [(s, 3, 0) for s in SL.SIZES],
        "65 small tensors": [(s[0], 3, 0) for s in SL.MANY],
        "an empty tensor is not there": [(0, 3, 0), (5, 1, 0), (0, 1, 0)],
        "only empty tensors": [(0, 3, 0)],
        "stepped only and clipped only": [(4, 2, 0), (6, 1, 0)],
        "2^31 elements": [(1 << 30, 1, 0)] * 2,
        "the shipped sizes": [(s, 3, 0) for s in (16 * 9, 16, 48 * 16, 48, 192 * 64, 64, 64, 64 * 64, 25 * 64, 25)],
    }
    for what, ts in cases.items():
        assert lib.gmpe_optim_shard_elems(C.byref(_plan(ts)), C.byref(n)) == 0, (what, lib.gmpe_last_error())
        assert n.value == SL.elems(ts), (what, n.value)
    assert SL.elems(cases["the test shapes"]) == 7172 and SL.elems(cases["65 small tensors"]) == 13 * 15 and len(SL.MANY) == OL.MAX_TENSORS + 1
    assert len(OL.geometry([(s[0], 3, 0) for s in SL.MANY])) == 2          # the 65 tensors span two launch groups
    starts = np.cumsum((0,) + SL.SIZES[:-1])
    assert (starts[1:] % 4 != 0).all() and sum(a // OL.CHUNK != (a + s - 1) // OL.CHUNK for a, s in zip(starts, SL.SIZES)) >= 3
    assert lib.gmpe_optim_shard_elems(C.byref(_plan([(1, 3, 0)])), None) == -1 and "elems_out" in lib.gmpe_last_error().decode()
    assert lib.gmpe_optim_shard_elems(None, C.byref(n)) == -1 and lib.gmpe_last_error().decode() == "gmpe_optim_shard_elems: null plan"
    assert lib.gmpe_optim_shard_elems(C.byref(_plan([(-1, 3, 0)])), C.byref(n)) == -1 and "tensors[0].numel" in lib.gmpe_last_error().decode()


def test_the_restated_rule_tells_rank_orders_and_precisions_apart():
    f = lambda *x: [np.array([v], np.float32) for v in x]
    assert SL.BIG == (2.0 ** 60, -2.0 ** 60, 1.0) and SL.SWAPPED == (2.0 ** 60, 1.0, -2.0 ** 60)
    assert SL.fold(f(*SL.BIG))[0] == 1.0 and SL.fold(f(*SL.SWAPPED))[0] == 0.0
    # the cancellation row: float32(-1e8 + 3) is -1e8 (the spacing there is 8), so what is left is rank 2's 0.25 — a fold that skips a rank shows here
    assert SL.fold(f(*SL.CANCEL))[0] == 0.25
    # float32 adds lose what the double fold keeps: 1e8 + 3 is a double but no float32
    row = f(*SL.KEEPS)
    in_f32 = np.float32(np.float32(row[0][0] + row[1][0]) + row[2][0])
    assert SL.fold(row)[0] == 3.0 and in_f32 == 0.0
    # the fold starts at rank 0's value: a negative zero stays one
    assert np.signbit(SL.fold(f(-0.0, -0.0))[0]) and not np.signbit(SL.fold(f(-0.0, 0.0))[0])
    # one rank is the identity, bit for bit
    g = OL.gradients(SL.SHAPES, 0)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(SL.summed([g]), g))
    per_rank = SL.rank_gradients(SL.SHAPES, 3, 0)
    assert not np.array_equal(per_rank[0][1], per_rank[1][1]) and SL.summed(per_rank)[4].dtype == np.float32


def _handle(n=5, done=False, extra=False):
    carry = (torch.zeros(2), torch.zeros(6)) if extra else None
    h = gmpe.optim.ClipAndStepShard(None, [], [], torch.device("cpu"), False, 0.0, True, carry, None, torch.zeros(n))
    h.done = done
    return h


@pytest.mark.parametrize("make,match", [
    (lambda: torch.zeros(2, 5, dtype=torch.float64), "must be float32, not torch.float64"), (lambda: torch.zeros(2, 4), r"shape \(world, 5\)"),
    (lambda: torch.zeros(10), r"shape \(world, 5\)"), (lambda: torch.zeros(5, 2).t(), "contiguous"), (lambda: torch.zeros(2, 5, device="meta"), "must be on cpu"),
    (lambda: torch.zeros(0, 5), "world = 0"), (lambda: np.zeros((2, 5), np.float32), r"shape \(world, 5\)")])
def test_finish_checks_all_before_any_launch(make, match):
    h = _handle()
    with pytest.raises(ValueError, match=match):
        gmpe.clip_and_step_finish(h, make())
    assert not h.done


def test_python_refusals_come_before_any_device_call():
    with pytest.raises(RuntimeError, match="already called"):
        gmpe.clip_and_step_finish(_handle(done=True), torch.zeros(2, 5))
    with pytest.raises(TypeError, match="clip_and_step_begin"):
        gmpe.clip_and_step_finish(object(), torch.zeros(2, 5))
    ps, opt = _adam()
    with pytest.raises(ValueError, match="CUDA"):                       # CPU tensors: clip_and_step's own refusal, in begin
        gmpe.clip_and_step_begin(opt, 10.0)
    with pytest.raises(ValueError, match="at most 16 elements, not 17"):
        gmpe.clip_and_step_begin(opt, 10.0, extra=torch.zeros(17))
    for bad in (torch.zeros(3, dtype=torch.float64), [1.0, 2.0], torch.zeros(3, dtype=torch.int32)):
        with pytest.raises(ValueError, match="extra must be a float32 tensor"):
            gmpe.clip_and_step_begin(opt, 10.0, extra=bad)
    with pytest.raises(ValueError, match="extra rides on the exchange"):
        gmpe.clip_and_step(opt, 10.0, extra=torch.zeros(3))
    with pytest.raises(ValueError, match="max_grad_norm must be positive"):
        gmpe.clip_and_step_begin(opt, -1.0)
    with pytest.raises(NotImplementedError, match="amsgrad"):
        gmpe.clip_and_step_begin(_adam(amsgrad=True)[1], 10.0)
    assert all(not opt.state[p] for p in ps)
    # a `shards` that is no exchange: clip_and_step says so as the other shards= arguments do, ppo_update and train before anything else is read
    args = types.SimpleNamespace()
    half = types.SimpleNamespace(exchange=lambda local: local, world=2)                      # no rank
    for bad in (object(), half):
        with pytest.raises(TypeError, match="exchange"):
            gmpe.clip_and_step(opt, 10.0, shards=bad)
        with pytest.raises(NotImplementedError, match="shards.*exchange.*world.*rank.*anything else is not supported"):
            policy.ppo_update(None, None, None, None, (None,) * 16, args, shards=bad)
        with pytest.raises(NotImplementedError, match="shards.*anything else is not supported"):
            policy.train(None, None, None, None, None, args, shards=bad)
    ok = types.SimpleNamespace(exchange=lambda local: local, world=2, rank=0)
    with pytest.raises(NotImplementedError, match="accumulation_steps"):
        policy.ppo_update(None, None, None, None, (None,) * 16, args, shards=ok, accumulation_steps=2)
    with pytest.raises(NotImplementedError, match="accumulation_steps"):
        policy.train(None, None, None, None, None, args, shards=ok, accumulation_steps=3)
    with pytest.raises(ValueError, match="shards.world must be in"):
        gmpe.clip_and_step(opt, 10.0, shards=types.SimpleNamespace(exchange=lambda local: local, world=0, rank=0))


def test_check_all_stats_keeps_its_float64_behaviour():
    local = torch.zeros(3, dtype=torch.float64)
    assert learner_shards.check_all_stats(torch.zeros(4, 3, dtype=torch.float64), local, "x") == 4
    with pytest.raises(ValueError, match="x: all_stats must be float64, not torch.float32"):
        learner_shards.check_all_stats(torch.zeros(4, 3), local, "x")
    assert learner_shards.check_all_stats(torch.zeros(4, 3), local.float(), "x", torch.float32) == 4
    with pytest.raises(ValueError, match="x: all_stats must be float32, not torch.float64"):
        learner_shards.check_all_stats(torch.zeros(4, 3, dtype=torch.float64), local.float(), "x", torch.float32)


def test_the_lockstep_exchange_stacks_in_rank_order_and_a_failure_ends_the_others():
    x = SL.Lockstep(3, timeout=20.0)
    out = x.run(lambda r, sh: [sh.exchange(torch.full((2,), float(10 * k + r))) for k in range(3)])
    for r in range(3):
        for k in range(3):
            assert out[r][k].tolist() == [[10.0 * k + q] * 2 for q in range(3)]
    assert x.calls == [3, 3, 3] and learner_shards.check_shards(x.rank(1)) == 3

    def body(r, sh):
        if r == 1:
            raise KeyError("replica 1")
        return sh.exchange(torch.zeros(1))

    with pytest.raises(KeyError, match="replica 1"):
        SL.Lockstep(3, timeout=20.0).run(body)


def test_the_new_kernels_use_no_scratch():
    assert "optimshard" in abi_lib.ru_objects()                                   # `make resource-usage` holds it
    found = abi_lib.scratch("optimshard")
    assert len(found) == 2 and all(v == 0 for v in found.values()), found
    assert any("k_opt_pack" in k for k in found) and any("k_opt_reduce" in k for k in found)
