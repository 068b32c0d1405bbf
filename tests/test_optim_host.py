"""Host side of the gradient clip and the Adam step (include/gmpe.h gmpe_optim_workspace_bytes / gmpe_optim_step, gmpe.clip_and_step), no GPU:
(a) tests/optim_lib.py's float64 restatement is torch's clip_grad_norm_ + Adam.step: it agrees with torch's float64 run on the CPU to 1e-12 over five
    steps, and torch's float32 run of the accuracy construction stays under the 1e-5 cap for every array;
(b) the exported symbols, the structs' layout against the C header, the workspace size against the restated geometry, the refusals of both layers —
    every one before any device call (where there is no device, a call that got that far fails with a HIP error instead);
(c) the compiler's resource report of csrc/gmpe_optim.hip shows no scratch memory."""
import ctypes as C

import numpy as np
import pytest
import torch

import abi_lib
import gmpe
import optim_lib as OL
from gmpe import _lib

MB = 1 << 20


# ---------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_the_restatement_is_torchs_clip_and_adam_in_float64(wd):
    params = OL.parameters(OL.SHAPES)
    truth = OL.restated_steps(params, OL.SHAPES, OL.STEPS, wd)
    t64 = OL.torch_steps([p.astype(np.float64) for p in params], OL.SHAPES, OL.STEPS, torch.float64, wd)
    for k in range(OL.STEPS):
        e = OL.errors(t64[k], truth[k])
        print("wd %g step %d" % (wd, k), {a: "%.3g" % x for a, x in e.items()})
        assert max(e.values()) <= 1e-12, (k, e)
    assert truth[0]["norm"] > OL.MAX_NORM > truth[1]["norm"] > 1.0          # the first step is clipped, the later ones are not


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_torchs_float32_run_stays_under_the_cap(wd):
    params = OL.parameters(OL.SHAPES)
    truth = OL.restated_steps(params, OL.SHAPES, OL.STEPS, wd)
    r32 = OL.torch_steps(params, OL.SHAPES, OL.STEPS, torch.float32, wd)
    for k in range(OL.STEPS):
        e = OL.errors(r32[k], truth[k])
        print("wd %g step %d err_ref" % (wd, k), {a: "%.3g" % x for a, x in e.items()})
        assert max(e.values()) <= OL.CAP, (k, e)


def test_the_metric_is_relative_to_the_arrays_own_size():
    t = np.array([1e-6, -2e-6])
    assert OL.err(t * (1 + 1e-3), t) == pytest.approx(1e-3) and OL.err(t, t) == 0.0 and OL.err(np.zeros(0), np.zeros(0)) == 0.0
    assert OL.bound(0.0) == 2.0 ** -23 and OL.bound(1e-7) == 4e-7 + 2.0 ** -23


# ---------------------------------------------------------------------------------------------- (b)
def test_symbols_are_exported_and_the_structs_match_the_header():
    lib = _lib.load()
    assert {"gmpe_optim_workspace_bytes", "gmpe_optim_step"} <= set(_lib.SYMBOLS) & abi_lib.exported()
    assert lib.gmpe_abi_version() == 3 and gmpe.config.ABI_VERSION == 3          # added entry points: the ABI version stays
    for cls in (_lib.GmpeOptimTensor, _lib.GmpeOptimHyper, _lib.GmpeOptimPlan):
        assert abi_lib.layout(cls) == abi_lib.mirror_layout(cls), cls
    assert C.sizeof(_lib.GmpeOptimTensor) == 48 and C.sizeof(_lib.GmpeOptimHyper) == 48
    names = ("MAX_TENSORS", "MAX_HYPERS", "CHUNK", "MAX_PLAN_TENSORS", "MAX_NUMEL", "CLIP", "STEP", "T_IN_NORM", "T_STEP")
    got = [abi_lib.constant("GMPE_OPT_" + k) for k in names]
    assert got + [abi_lib.constant("GMPE_ABI_VERSION")] == [64, 8, 1024, 4096, 1 << 30, 1, 2, 1, 2, 3]
    assert got == [getattr(_lib, "OPT_" + k) for k in names]
    assert (OL.CHUNK, OL.MAX_TENSORS, OL.MAX_HYPERS, OL.IN_NORM, OL.STEP) == (1024, 64, 8, 1, 2) and gmpe.optim.CHUNK == 1024
    # 64 descriptors of 40 bytes and 8 hyper-parameter sets of 28 bytes travel as kernel arguments: under 4 KB with everything else
    assert 64 * 40 + 8 * 28 + 8 + 64 <= 4096
    assert gmpe.clip_and_step is gmpe.optim.clip_and_step
    for name in ("ppo_update", "train"):
        assert callable(getattr(gmpe.policy, name))


def _plan(table, sets=((1e-3, 0.9, 0.999, 1e-8, 0.0, 1),), flags=3, max_norm=10.0, **over):
    """a plan over fake, well separated addresses: nothing here reaches a device. table: [(numel, flags, hyper)] or dicts of fields; sets: the hypers"""
    n, hypers = len(table), sets
    ts = (_lib.GmpeOptimTensor * max(n, 1))()
    for i, t in enumerate(table):
        t = dict(zip(("numel", "flags", "hyper"), t)) if isinstance(t, tuple) else t
        base = (4 * i + 1) * 16 * MB
        ts[i].param, ts[i].grad, ts[i].exp_avg, ts[i].exp_avg_sq = base, base + 4 * MB, base + 8 * MB, base + 12 * MB
        for k, v in t.items():
            setattr(ts[i], k, v)
    hs = (_lib.GmpeOptimHyper * max(len(hypers), 1))()
    for i, h in enumerate(hypers):
        hs[i].lr, hs[i].beta1, hs[i].beta2, hs[i].eps, hs[i].weight_decay, hs[i].t = h
    p = _lib.GmpeOptimPlan()
    p.n_tensors, p.n_hypers, p.tensors, p.hypers, p.flags, p.max_norm = n, len(hypers), ts, hs, flags, max_norm
    p.out, p.grad_norm_f32, p.workspace, p.workspace_bytes = 8, 64, 1 << 40, 1 << 30
    for k, v in over.items():
        setattr(p, k, v)
    p._keep = (ts, hs)
    return p


def test_workspace_bytes_and_the_restated_geometry():
    lib = _lib.load()
    n = C.c_size_t(7)
    Cn, M = OL.CHUNK, OL.MAX_TENSORS
    cases = {
        "one element": ([(1, 3, 0)], 8),
        "a chunk and its neighbours": ([(Cn - 1, 3, 0), (Cn, 3, 0), (Cn + 1, 3, 0)], 8 * 3),        # 3 * Cn elements concatenated: exactly three chunks
        "an empty tensor is not there": ([(0, 3, 0), (5, 1, 0), (0, 1, 0)], 8),
        "only empty tensors": ([(0, 3, 0)], 0),
        "M tensors": ([(3, 3, 0)] * M, 8),
        "M + 1 tensors": ([(3, 3, 0)] * (M + 1), 16),
        "2M + 1 tensors": ([(3, 3, 0)] * (2 * M + 1), 24),
        "a ninth hyper set opens a group": ([(3, 3, k) for k in range(9)], 16),
        "norm-only tensors bring no hyper set": ([(3, 3, k) for k in range(8)] + [(3, 1, 0)] * 5, 8),
        "2^31 elements do not fit one group": ([(1 << 30, 1, 0)] * 2, 8 * 2 * (1 << 20)),
        "the shipped sizes": ([(s, 3, 0) for s in (16 * 9, 16, 48 * 16, 48, 192 * 64, 64, 64, 64 * 64, 25 * 64, 25)], 8 * 19),
    }
    for what, (ts, want) in cases.items():
        nh = max(h for _, _, h in ts) + 1
        plan = _plan(ts, sets=((1e-3, 0.9, 0.999, 1e-8, 0.0, 1),) * nh)
        assert lib.gmpe_optim_workspace_bytes(C.byref(plan), C.byref(n)) == 0, (what, lib.gmpe_last_error())
        assert n.value == OL.workspace_bytes(ts) == want and n.value % 8 == 0, (what, n.value, OL.workspace_bytes(ts))
    assert OL.geometry([(3, 3, 0)] * (M + 1)) == [(M, 3 * M, 1), (1, 3, 1)] and OL.geometry([(0, 3, 0)]) == [(0, 0, 0)]
    assert lib.gmpe_optim_workspace_bytes(C.byref(_plan([(1, 3, 0)])), None) == -1 and "bytes_out" in lib.gmpe_last_error().decode()
    assert lib.gmpe_optim_workspace_bytes(None, C.byref(n)) == -1 and "null plan" in lib.gmpe_last_error().decode()


def test_the_python_bound_covers_every_subset_of_the_tensors():
    rng = np.random.RandomState(5)
    for trial in range(50):
        sizes = [int(x) for x in rng.choice([0, 1, 3, 1023, 1024, 1025, 4000], size=rng.randint(1, 140))]
        ps = [torch.nn.Parameter(torch.zeros(s)) for s in sizes]
        opt = torch.optim.Adam([dict(params=ps[:len(ps) // 2 + 1]), dict(params=ps[len(ps) // 2 + 1:], lr=0.1)] if len(ps) > 1 else ps)
        bound = gmpe.optim.workspace_bytes(opt)
        for _ in range(4):
            have = rng.rand(len(ps)) > 0.3
            ts = [(s, 3, int(i > len(ps) // 2)) for i, (s, h) in enumerate(zip(sizes, have)) if h]
            assert OL.workspace_bytes(ts) <= bound, (sizes, have)


C_REFUSALS = [
    (dict(n_tensors=0), "n_tensors"), (dict(n_tensors=4097), "n_tensors"), (dict(n_hypers=-1), "n_hypers"), (dict(tensors=None), "tensors is null"),
    (dict(hypers=None), "hypers is null"), (dict(flags=4), "flags"), (dict(reserved=1), "reserved"), (dict(max_norm=0.0), "max_norm"),
    (dict(max_norm=-1.0), "max_norm"), (dict(max_norm=float("nan")), "max_norm"), (dict(out=None), "out is required"), (dict(out=12), "out must be 8-byte"),
    (dict(grad_norm_f32=66), "grad_norm_f32"), (dict(workspace=None), "workspace is required"), (dict(workspace=(1 << 40) + 4), "workspace must be 8-byte"),
    (dict(workspace_bytes=8), "workspace_bytes is below gmpe_optim_workspace_bytes(plan) = 16"),
]
T_REFUSALS = [
    (dict(numel=-1), "tensors[1].numel"), (dict(numel=(1 << 30) + 1), "tensors[1].numel"), (dict(flags=0), "tensors[1].flags"), (dict(flags=4), "tensors[1].flags"),
    (dict(hyper=1), "tensors[1].hyper"), (dict(hyper=-1), "tensors[1].hyper"), (dict(flags=1, hyper=1), "tensors[1].hyper"),
    (dict(param=None), "tensors[1].param is required"), (dict(param=MB + 2), "tensors[1].param must be 4-byte"), (dict(grad=None), "tensors[1].grad is required"),
    (dict(grad=MB + 1), "tensors[1].grad must be 4-byte"), (dict(exp_avg=None), "tensors[1].exp_avg is required"), (dict(exp_avg=MB + 3), "tensors[1].exp_avg must"),
    (dict(exp_avg_sq=None), "tensors[1].exp_avg_sq is required"), (dict(exp_avg_sq=MB + 2), "tensors[1].exp_avg_sq must"),
]
H_REFUSALS = [
    ((-1e-3, 0.9, 0.999, 1e-8, 0.0, 1), "hypers[0].lr"), ((float("nan"), 0.9, 0.999, 1e-8, 0.0, 1), "hypers[0].lr"), ((1e-3, 1.0, 0.999, 1e-8, 0.0, 1), "hypers[0].beta1"),
    ((1e-3, -0.1, 0.999, 1e-8, 0.0, 1), "hypers[0].beta1"), ((1e-3, 0.9, 1.0, 1e-8, 0.0, 1), "hypers[0].beta2"), ((1e-3, 0.9, -1.0, 1e-8, 0.0, 1), "hypers[0].beta2"),
    ((1e-3, 0.9, 0.999, -1e-8, 0.0, 1), "hypers[0].eps"), ((1e-3, 0.9, 0.999, 1e-8, -0.1, 1), "hypers[0].weight_decay"), ((1e-3, 0.9, 0.999, 1e-8, 0.0, 0), "hypers[0].t"),
]


def test_the_c_entry_refuses_before_any_launch():
    lib = _lib.load()
    two = [(CHUNK_PLUS, 3, 0) for CHUNK_PLUS in (OL.CHUNK + 1, 7)]           # 1032 elements: two chunks, 16 bytes
    refused = lambda plan: (lib.gmpe_optim_step(0, C.byref(plan) if plan is not None else None, None), lib.gmpe_last_error().decode())
    rc, msg = refused(None)
    assert rc == -1 and msg == "gmpe_optim_step: null plan"
    for over, field in C_REFUSALS:
        rc, msg = refused(_plan(two, **over))
        assert rc == -1 and msg.startswith("gmpe_optim_step: ") and field in msg, (over, msg)
    for over, field in T_REFUSALS:
        rc, msg = refused(_plan([two[0], dict(dict(zip(("numel", "flags", "hyper"), two[1])), **over)]))
        assert rc == -1 and msg.startswith("gmpe_optim_step: ") and field in msg, (over, msg)
    for h, field in H_REFUSALS:
        rc, msg = refused(_plan(two, sets=(h,)))
        assert rc == -1 and msg.startswith("gmpe_optim_step: ") and field in msg, (h, msg)
    # what a call does not use is not asked for: no max_norm without GMPE_OPT_CLIP, no param or state without GMPE_OPT_STEP or for an empty tensor —
    # such a plan passes every check and, where there is no device, fails only at the device
    if not torch.cuda.is_available():
        for plan in (_plan(two, flags=2, max_norm=-1.0), _plan([(5, 3, 0)], flags=1, workspace_bytes=8),
                     _plan([dict(numel=5, flags=3, hyper=0, param=None, exp_avg=None, exp_avg_sq=None)], flags=1),
                     _plan([(5, 1, 0), dict(numel=0, flags=3, hyper=0, param=None, grad=None, exp_avg=None, exp_avg_sq=None)])):
            rc, msg = refused(plan)
            assert rc != 0 and msg.startswith("hip"), msg


def _adam(n=2, **kw):
    ps = [torch.nn.Parameter(torch.zeros(4, 3)) for _ in range(n)]
    for p in ps:
        p.grad = torch.ones(4, 3)
    return ps, torch.optim.Adam(ps, **kw)


def test_clip_and_step_refuses_by_name_before_any_device_call():
    for kw, word in ((dict(amsgrad=True), "amsgrad"), (dict(maximize=True), "maximize"), (dict(capturable=True), "capturable"),
                     (dict(differentiable=True), "differentiable"), (dict(decoupled_weight_decay=True), "decoupled_weight_decay"),
                     (dict(lr=torch.tensor(1e-3)), "tensor hyper-parameter")):
        with pytest.raises(NotImplementedError, match=word):
            gmpe.clip_and_step(_adam(**kw)[1], 10.0)
    ps, opt = _adam()
    opt.param_groups[0]["fused"] = True                                 # torch refuses to build a fused Adam over CPU tensors; the flag is what is read
    with pytest.raises(NotImplementedError, match="fused"):
        gmpe.clip_and_step(opt, 10.0)
    with pytest.raises(NotImplementedError, match="AdamW.*not supported|decoupled_weight_decay"):
        gmpe.clip_and_step(torch.optim.AdamW(_adam()[0]), 10.0)
    with pytest.raises(NotImplementedError, match="SGD.*other optimisers are not supported"):
        gmpe.clip_and_step(torch.optim.SGD(_adam()[0], lr=0.1), 10.0)
    for dt in (torch.float16, torch.bfloat16):
        ps, opt = _adam()
        ps[1].data = ps[1].data.to(dt)
        ps[1].grad = ps[1].grad.to(dt)
        with pytest.raises(NotImplementedError, match="half precision"):
            gmpe.clip_and_step(opt, 10.0)
    ps, opt = _adam()
    ps[0].grad = torch.sparse_coo_tensor(torch.tensor([[0], [1]]), torch.tensor([1.0]), (4, 3))
    with pytest.raises(NotImplementedError, match="sparse"):
        gmpe.clip_and_step(opt, 10.0)
    ps, opt = _adam()
    ps[1].data, ps[1].grad = ps[1].data.double(), ps[1].grad.double()
    with pytest.raises(ValueError, match="parameter 1 must be float32"):
        gmpe.clip_and_step(opt, 10.0)
    ps, opt = _adam()
    ps[1].data = torch.zeros(3, 4).t()
    with pytest.raises(ValueError, match="parameter 1 must be contiguous"):
        gmpe.clip_and_step(opt, 10.0)
    ps, opt = _adam()
    opt.step()
    opt.state[ps[0]]["exp_avg_sq"] = torch.zeros(3, 4).t()
    with pytest.raises(ValueError, match=r"state\['exp_avg_sq'\] must be contiguous"):
        gmpe.clip_and_step(opt, 10.0)
    gmpe_step_false = _adam()
    gmpe_step_false[1].step()
    gmpe_step_false[1].state[gmpe_step_false[0][0]]["exp_avg"] = torch.zeros(3, 4).t()
    with pytest.raises(ValueError, match="CUDA"):                       # step=False does not look at the state: the next refusal is the device's
        gmpe.clip_and_step(gmpe_step_false[1], 10.0, step=False)
    ps = [torch.nn.Parameter(torch.zeros(4, 3, device=d)) for d in ("cpu", "meta")]          # tensors on different devices
    for p in ps:
        p.grad = torch.zeros_like(p)
    opt = torch.optim.Adam(ps)
    with pytest.raises(ValueError, match="parameter 1 is on meta: every tensor must be on cpu"):
        gmpe.clip_and_step(opt, 10.0)
    ps, opt = _adam()
    extra = torch.nn.Parameter(torch.zeros(2, device="meta"))
    extra.grad = torch.zeros(2, device="meta")
    with pytest.raises(ValueError, match=r"parameters\[2\] is on meta"):
        gmpe.clip_and_step(opt, 10.0, parameters=ps + [extra])
    ps, opt = _adam()
    with pytest.raises(ValueError, match="CUDA"):                       # CPU tensors
        gmpe.clip_and_step(opt, 10.0)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_grad_norm must be positive"):
            gmpe.clip_and_step(opt, bad)
    with pytest.raises(ValueError, match=r"parameters\[0\] must be a tensor"):
        gmpe.clip_and_step(opt, 10.0, parameters=[3.0])
    with pytest.raises(ValueError, match="hold no tensor"):
        gmpe.clip_and_step(torch.optim.Adam([dict(params=[])]), 10.0)
    assert all(not opt.state[p] for p in ps)                            # and nothing was created or counted on the way


def test_created_state_is_torchs():
    """the state clip_and_step creates for a tensor: torch's keys, dtypes, shapes and devices, as Adam.step creates them (the same function on a device)"""
    ps, opt = _adam()
    opt.step()
    for p in ps:
        st = {}
        gmpe.optim._new_state(st, p)
        want = opt.state[p]
        assert list(st) == list(want) == ["step", "exp_avg", "exp_avg_sq"]
        for k in st:
            assert st[k].dtype == want[k].dtype and st[k].device == want[k].device and st[k].shape == want[k].shape and not st[k].requires_grad, k
            assert float(st[k].abs().sum()) == 0.0
        assert st["step"].device.type == "cpu" and st["step"].dim() == 0 and st["step"].dtype == torch.float32


def test_ppo_update_and_train_refuse_what_they_do_not_do():
    import types
    from gmpe import policy
    args = types.SimpleNamespace()
    with pytest.raises(NotImplementedError, match="accumulation_steps"):
        policy.ppo_update(None, None, None, None, (None,) * 16, args, accumulation_steps=2)
    with pytest.raises(NotImplementedError, match="shards"):
        policy.ppo_update(None, None, None, None, (None,) * 16, args, shards=object())
    with pytest.raises(NotImplementedError, match="accumulation_steps"):
        policy.train(None, None, None, None, None, args, accumulation_steps=2)
    assert policy.TRAIN_INFO == ("value_loss", "policy_loss", "dist_entropy", "actor_grad_norm", "critic_grad_norm", "ratio")
    assert policy.PPOUpdate._fields == ("value_loss", "critic_grad_norm", "policy_loss", "dist_entropy", "actor_grad_norm", "ratio_mean", "imp_weights")


# ---------------------------------------------------------------------------------------------- (c)
def test_the_kernels_use_no_scratch():
    found = abi_lib.scratch("optim")
    assert len(found) == 2 and all(v == 0 for v in found.values()), found
    assert any("k_opt_norm" in k for k in found) and any("k_opt_step" in k for k in found)
