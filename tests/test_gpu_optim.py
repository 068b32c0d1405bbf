"""gmpe.clip_and_step (include/gmpe.h gmpe_optim_step) on the device against tests/optim_lib.py's float64 restatement of clip_grad_norm_ + Adam.step, by
the project's accuracy rule per array — err_dev <= 4 * err_ref + 2^-23 with err_ref <= 1e-5, err_ref from torch's float32 run of the same steps on the
CPU, err relative to the array's own size — and bit for bit where the contract says so. C is the chunk size (1024), M the tensors per launch (64)."""
import ctypes as C

import numpy as np
import pytest
import torch

import gmpe
import optim_lib as OL
from gmpe import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = OL.ARRAYS + ("norm",)


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def holds(dev, ref, truth, what):
    """the accuracy rule for every array of one step's snapshots"""
    e_dev, e_ref = OL.errors(dev, truth), OL.errors(ref, truth)
    for k in KINDS:
        print("%s %-10s err_ref %.3g err_dev %.3g bound %.3g" % (what, k, e_ref[k], e_dev[k], OL.bound(e_ref[k])))
    for k in KINDS:
        assert e_ref[k] <= OL.CAP and e_dev[k] <= OL.bound(e_ref[k]), (what, k, e_dev[k], e_ref[k])


def device_steps(params, shapes, steps, weight_decay, max_norm=OL.MAX_NORM, seed=0, workspace=None):
    ps = OL.torch_params(params, device=DEV)
    opt = torch.optim.Adam(ps, lr=OL.LR, eps=OL.EPS, weight_decay=weight_decay)
    out = []
    for k in range(steps):
        OL.set_grads(ps, OL.gradients(shapes, k, seed))
        norm = gmpe.clip_and_step(opt, max_norm, workspace=workspace)
        assert norm.dtype == torch.float32 and norm.dim() == 0 and norm.device == ps[0].device
        out.append(OL.snapshot(ps, opt, norm))
    return out, ps, opt


# ---------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_five_steps_meet_the_accuracy_rule(wd):
    params = OL.parameters(OL.SHAPES)
    truth = OL.restated_steps(params, OL.SHAPES, OL.STEPS, wd)
    ref = OL.torch_steps(params, OL.SHAPES, OL.STEPS, torch.float32, wd)
    ws = torch.empty(1 << 12, dtype=torch.uint8, device=DEV)
    dev, ps, opt = device_steps(params, OL.SHAPES, OL.STEPS, wd, workspace=ws)
    assert truth[0]["norm"] > OL.MAX_NORM > truth[1]["norm"]                # clipped, then not
    for k in range(OL.STEPS):
        holds(dev[k], ref[k], truth[k], "wd %g step %d" % (wd, k))
    assert all(float(opt.state[p]["step"]) == OL.STEPS and opt.state[p]["step"].device.type == "cpu" for p in ps)
    assert gmpe.optim.workspace_bytes(opt) <= ws.numel()


# ---------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("n", [1, OL.MAX_TENSORS, OL.MAX_TENSORS + 1, 2 * OL.MAX_TENSORS + 1])
def test_tensor_count_edges(n):
    shapes, MN = ((3,),) * n, 0.01                    # the lone first tensor has the smallest gradients: its norm is about 0.05
    params = OL.parameters(shapes, seed=n)
    truth = OL.restated_steps(params, shapes, 3, 1e-2, max_norm=MN, seed=n)
    ref = OL.torch_steps(params, shapes, 3, torch.float32, 1e-2, max_norm=MN, seed=n)
    dev, ps, opt = device_steps(params, shapes, 3, 1e-2, max_norm=MN, seed=n)
    assert truth[0]["norm"] > MN
    for k in range(3):
        holds(dev[k], ref[k], truth[k], "%d tensors step %d" % (n, k))
    # the norm covers every group: all-ones gradients have the norm sqrt(3 n), an exact sum, which every single tensor changes
    OL.set_grads(ps, [np.ones(3, np.float32)] * n)
    assert float(gmpe.clip_and_step(opt, None, step=False)) == float(np.float32(np.sqrt(3.0 * n)))


# ---------------------------------------------------------------------------------------------- 3
def test_equal_state_gives_equal_bits_and_a_tensor_steps_as_if_alone():
    shapes = OL.SHAPES
    params = OL.parameters(shapes, seed=3)
    runs = [device_steps(params, shapes, 2, 1e-2, seed=3) for _ in range(2)]
    for k in range(2):
        for kind in OL.ARRAYS:
            for a, b in zip(runs[0][0][k][kind], runs[1][0][k][kind]):
                assert same(a, b), (k, kind)
        assert runs[0][0][k]["norm"] == runs[1][0][k]["norm"]
    # max_grad_norm=None: the gradients keep their bits, and every tensor gets the bits of stepping it alone
    grads = OL.gradients(shapes, 0, 3)
    ps = OL.torch_params(params, device=DEV)
    opt = torch.optim.Adam(ps, lr=OL.LR, eps=OL.EPS, weight_decay=1e-2)
    OL.set_grads(ps, grads)
    norm = gmpe.clip_and_step(opt, None)
    want = float(np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in grads)))
    assert float(norm) == np.float32(want)
    for i in (0, 2, 4, 6, 9):
        alone = OL.torch_params([params[i]], device=DEV)
        opt1 = torch.optim.Adam(alone, lr=OL.LR, eps=OL.EPS, weight_decay=1e-2)
        OL.set_grads(alone, [grads[i]])
        gmpe.clip_and_step(opt1, None)
        assert same(alone[0], ps[i]) and same(opt1.state[alone[0]]["exp_avg"], opt.state[ps[i]]["exp_avg"])
        assert same(opt1.state[alone[0]]["exp_avg_sq"], opt.state[ps[i]]["exp_avg_sq"])
        assert not same(alone[0], params[i])
    for p, g in zip(ps, grads):
        assert same(p.grad, g)


# ---------------------------------------------------------------------------------------------- 4
def test_views_at_odd_float_offsets_and_their_guards():
    sizes = (5, OL.CHUNK - 1, OL.CHUNK + 1, 2 * OL.CHUNK + 3)
    shapes = tuple((s,) for s in sizes)
    params, grads = OL.parameters(shapes, seed=4), OL.gradients(shapes, 0, 4)
    plain, _, _ = device_steps(params, shapes, 1, 1e-2, seed=4)
    GUARD = 7.25
    offs = {"param": 3, "grad": 5, "exp_avg": 1, "exp_avg_sq": 7}
    bufs = {k: [torch.full((s + 16,), GUARD, device=DEV) for s in sizes] for k in offs}
    view = lambda k, i: bufs[k][i][offs[k]:offs[k] + sizes[i]]
    ps = []
    for i, s in enumerate(sizes):
        view("param", i).copy_(torch.from_numpy(params[i]))
        view("grad", i).copy_(torch.from_numpy(grads[i]))
        view("exp_avg", i).zero_()
        view("exp_avg_sq", i).zero_()
        p = torch.nn.Parameter(view("param", i))
        p.grad = view("grad", i)
        assert p.data_ptr() % 16 != 0 and p.grad.data_ptr() % 16 != 0 and p.data_ptr() == bufs["param"][i].data_ptr() + 4 * offs["param"]
        ps.append(p)
    opt = torch.optim.Adam(ps, lr=OL.LR, eps=OL.EPS, weight_decay=1e-2)
    for i, p in enumerate(ps):
        opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": view("exp_avg", i), "exp_avg_sq": view("exp_avg_sq", i)}
    norm = gmpe.clip_and_step(opt, OL.MAX_NORM)
    torch.cuda.synchronize()
    assert float(norm) == np.float32(plain[0]["norm"])
    for i, s in enumerate(sizes):
        for k in offs:
            whole = bufs[k][i].cpu().numpy()
            assert (whole[:offs[k]] == GUARD).all() and (whole[offs[k] + s:] == GUARD).all(), (k, i)
            assert same(whole[offs[k]:offs[k] + s], plain[0][k][i]), (k, i)      # the bits do not depend on where the arrays lie


# ---------------------------------------------------------------------------------------------- 5
def _sets(device, dtype=torch.float32):
    shapes = ((7,), (40, 30), (OL.CHUNK + 5,), (33,), (0,))
    params, grads = OL.parameters(shapes, seed=5), OL.gradients(shapes, 0, 5)
    a, b, c, d, e = ps = OL.torch_params(params, dtype, device)
    OL.set_grads(ps, [None] + grads[1:])
    return params, grads, ps, torch.optim.Adam([a, b, d, e], lr=OL.LR, eps=OL.EPS), [a, b, c, e]


def test_the_clipped_set_and_the_stepped_set_may_differ():
    """a: no gradient; b: in both; c: in `parameters` only; d: in the optimiser only; e: no elements"""
    params, grads, ps, opt, normed = _sets(DEV)
    max_norm = 2.0
    norm = gmpe.clip_and_step(opt, max_norm, parameters=normed)
    a, b, c, d, e = ps
    # torch on the CPU, float32, and the restatement
    _, _, rps, ropt, rnormed = _sets("cpu")
    rnorm = torch.nn.utils.clip_grad_norm_(rnormed, max_norm)
    ropt.step()
    r = OL.Restated(params)
    tnorm, tg = r.step([None] + grads[1:], max_norm, in_norm=[True, True, True, False, True], stepped=[True, True, False, True, True])
    assert tnorm > max_norm
    f = lambda t: t.detach().double().cpu().numpy()
    for what, i in (("b", 1), ("c", 2), ("d", 3)):
        for kind, get in (("param", lambda q, o: f(q)), ("grad", lambda q, o: f(q.grad)), ("exp_avg", lambda q, o: f(o.state[q]["exp_avg"])),
                          ("exp_avg_sq", lambda q, o: f(o.state[q]["exp_avg_sq"]))):
            if what == "c" and kind.startswith("exp"):
                continue
            truth = {"param": r.p, "grad": tg, "exp_avg": r.m, "exp_avg_sq": r.v}[kind][i]
            e_ref, e_dev = OL.err(get(rps[i], ropt), truth), OL.err(get(ps[i], opt), truth)
            print("%s %-10s err_ref %.3g err_dev %.3g" % (what, kind, e_ref, e_dev))
            assert e_ref <= OL.CAP and e_dev <= OL.bound(e_ref), (what, kind, e_dev, e_ref)
    assert abs(float(norm) - tnorm) / tnorm <= OL.bound(abs(float(rnorm) - tnorm) / tnorm)
    assert same(a, params[0]) and a not in opt.state                       # no gradient: no state, no step
    assert same(c, params[2]) and c not in opt.state and not same(c.grad, grads[2])        # scaled only
    assert same(d.grad, grads[3]) and not same(d, params[3])               # stepped with its gradient as it was, and left out of the norm
    assert not same(b.grad, grads[1]) and not same(b, params[1])
    assert sorted(opt.state[e]) == ["exp_avg", "exp_avg_sq", "step"] and float(opt.state[e]["step"]) == 1 and opt.state[e]["exp_avg"].numel() == 0
    for p in (b, d):
        st = opt.state[p]
        assert list(st) == ["step", "exp_avg", "exp_avg_sq"] and float(st["step"]) == 1 and st["step"].device.type == "cpu"
        assert st["step"].dtype == torch.float32 and st["exp_avg"].device == p.device and st["exp_avg"].shape == p.shape
    # step=False clips only: no state, no step, the parameters keep their bits
    params, grads, ps, opt, normed = _sets(DEV)
    norm2 = gmpe.clip_and_step(opt, max_norm, parameters=normed, step=False)
    assert float(norm2) == float(norm) and len(opt.state) == 0
    assert all(same(p, q) for p, q in zip(ps, params)) and same(ps[1].grad, b.grad) and same(ps[2].grad, c.grad) and same(ps[3].grad, grads[3])
    # nothing has a gradient: the norm of nothing
    for p in ps:
        p.grad = None
    zero = gmpe.clip_and_step(opt, max_norm, parameters=normed)
    assert float(zero) == 0.0 and zero.dtype == torch.float32 and zero.device == ps[0].device and len(opt.state) == 0


# ---------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("ours_first", [True, False], ids=["ours-then-torch", "torch-then-ours"])
def test_interchange_with_torchs_own_step_through_state_dict(ours_first):
    shapes, wd = OL.SHAPES[:6], 1e-2
    params = OL.parameters(shapes, seed=6)
    truth = OL.restated_steps(params, shapes, 5, wd, seed=6)
    ref = OL.torch_steps(params, shapes, 5, torch.float32, wd, seed=6)
    ps = OL.torch_params(params, device=DEV)
    make = lambda: torch.optim.Adam(ps, lr=OL.LR, eps=OL.EPS, weight_decay=wd)

    def ours(opt, k):
        return gmpe.clip_and_step(opt, OL.MAX_NORM)

    def torchs(opt, k):
        norm = torch.nn.utils.clip_grad_norm_(ps, OL.MAX_NORM)
        opt.step()
        return norm

    first, second = (ours, torchs) if ours_first else (torchs, ours)
    n_first = 3 if ours_first else 2
    opt = make()
    for k in range(5):
        if k == n_first:
            fresh = make()
            fresh.load_state_dict(opt.state_dict())
            opt = fresh
        OL.set_grads(ps, OL.gradients(shapes, k, 6))
        norm = (first if k < n_first else second)(opt, k)
    assert all(float(opt.state[p]["step"]) == 5 for p in ps)
    holds(OL.snapshot(ps, opt, norm), ref[4], truth[4], "interchange")


# ---------------------------------------------------------------------------------------------- 7
def test_param_groups_and_a_changed_lr():
    shapes = OL.SHAPES[:6]
    params = OL.parameters(shapes, seed=7)
    cut = 3
    groups = lambda ps: [dict(params=ps[:cut]), dict(params=ps[cut:], lr=3e-3, eps=1e-3, weight_decay=5e-2)]
    lrs = (OL.LR, 4e-3, 4e-3)                          # the first group's lr at each step: changed between the first two calls
    r = OL.Restated(params)
    runs = {}
    for where in ("cpu", DEV):
        ps = OL.torch_params(params, device=where)
        opt = torch.optim.Adam(groups(ps), lr=OL.LR, eps=OL.EPS)
        for k in range(3):
            opt.param_groups[0]["lr"] = lrs[k]
            OL.set_grads(ps, OL.gradients(shapes, k, 7))
            if where == "cpu":
                norm = torch.nn.utils.clip_grad_norm_(ps, OL.MAX_NORM)
                opt.step()
            else:
                norm = gmpe.clip_and_step(opt, OL.MAX_NORM)
        runs[where] = OL.snapshot(ps, opt, norm)
    for k in range(3):
        norm, g = r.step(OL.gradients(shapes, k, 7), OL.MAX_NORM, lr=[lrs[k]] * cut + [3e-3] * (len(shapes) - cut),
                         eps=[OL.EPS] * cut + [1e-3] * (len(shapes) - cut), weight_decay=[0.0] * cut + [5e-2] * (len(shapes) - cut))
    truth = {"param": r.p, "grad": g, "exp_avg": r.m, "exp_avg_sq": r.v, "norm": norm}
    holds(runs[DEV], runs["cpu"], truth, "groups")
    # the restatement with one lr for all would be far off: the groups' own numbers were used
    one = OL.restated_steps(params, shapes, 3, 0.0, seed=7)[2]
    assert OL.errors(runs[DEV], one)["param"] > 1e-4


# ---------------------------------------------------------------------------------------------- 8
def test_an_infinite_gradient_entry_propagates_as_in_torch():
    shapes = ((6,), (OL.CHUNK + 2,), (9,))
    params, grads = OL.parameters(shapes, seed=8), OL.gradients(shapes, 0, 8)
    grads[1][OL.CHUNK] = np.inf
    got = {}
    for where in ("cpu", DEV):
        ps = OL.torch_params(params, device=where)
        opt = torch.optim.Adam(ps, lr=OL.LR, eps=OL.EPS)
        OL.set_grads(ps, grads)
        if where == "cpu":
            norm = torch.nn.utils.clip_grad_norm_(ps, OL.MAX_NORM)
            opt.step()
        else:
            norm = gmpe.clip_and_step(opt, OL.MAX_NORM)
        got[where] = ([p.detach().cpu().numpy() for p in ps], [p.grad.cpu().numpy() for p in ps], float(norm))
    assert got[DEV][2] == got["cpu"][2] == np.inf
    for i in range(3):
        for j in (0, 1):
            assert np.array_equal(np.isfinite(got[DEV][j][i]), np.isfinite(got["cpu"][j][i])) and np.array_equal(np.isnan(got[DEV][j][i]), np.isnan(got["cpu"][j][i]))
    assert np.isnan(got[DEV][1][1][OL.CHUNK]) and np.isnan(got[DEV][0][1][OL.CHUNK]) and np.isnan(got[DEV][1][1]).sum() == 1
    assert (got[DEV][1][0] == 0).all() and np.array_equal(got[DEV][0][0], params[0])      # the other gradients become 0: their parameters stay


# ---------------------------------------------------------------------------------------------- 9
def test_the_c_entry_on_a_side_stream_whatever_the_workspace_held():
    lib = _lib.load()
    shapes = ((5,), (OL.CHUNK + 1,), (77,))
    params, grads = OL.parameters(shapes, seed=9), OL.gradients(shapes, 0, 9)
    MN = 10.0                                          # under the norm of about 29: the clip bites
    want, _, _ = device_steps(params, shapes, 1, 1e-2, max_norm=MN, seed=9)
    stream = torch.cuda.Stream(device=DEV)
    GUARD = 0xA5
    results = []
    for fill in (0x00, 0xFF):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        p, g = [t(x) for x in params], [t(x) for x in grads]
        m, v = [torch.zeros_like(x) for x in p], [torch.zeros_like(x) for x in p]
        ts = (_lib.GmpeOptimTensor * 3)()
        for i in range(3):
            ts[i].param, ts[i].grad, ts[i].exp_avg, ts[i].exp_avg_sq = p[i].data_ptr(), g[i].data_ptr(), m[i].data_ptr(), v[i].data_ptr()
            ts[i].numel, ts[i].flags, ts[i].hyper = p[i].numel(), _lib.OPT_T_IN_NORM | _lib.OPT_T_STEP, 0
        hs = (_lib.GmpeOptimHyper * 1)()
        hs[0].lr, hs[0].beta1, hs[0].beta2, hs[0].eps, hs[0].weight_decay, hs[0].t = OL.LR, 0.9, 0.999, OL.EPS, 1e-2, 1
        plan = _lib.GmpeOptimPlan()
        plan.n_tensors, plan.n_hypers, plan.tensors, plan.hypers = 3, 1, ts, hs
        plan.flags, plan.max_norm = _lib.OPT_CLIP | _lib.OPT_STEP, MN
        need = C.c_size_t()
        assert lib.gmpe_optim_workspace_bytes(C.byref(plan), C.byref(need)) == 0 and need.value == OL.workspace_bytes([(x.size, 3, 0) for x in params]) == 16
        out = torch.full((64 + 16 + 64,), GUARD, dtype=torch.uint8, device=DEV)
        f32 = torch.full((64 + 8 + 64,), GUARD, dtype=torch.uint8, device=DEV)
        ws = torch.full((64 + need.value + 64,), GUARD, dtype=torch.uint8, device=DEV)
        ws[64:64 + need.value] = fill
        plan.out, plan.grad_norm_f32 = out.data_ptr() + 64, f32.data_ptr() + 64
        plan.workspace, plan.workspace_bytes = ws.data_ptr() + 64, need.value
        stream.wait_stream(torch.cuda.current_stream(DEV))
        rc = lib.gmpe_optim_step(0, C.byref(plan), C.c_void_p(stream.cuda_stream))
        assert rc == 0, lib.gmpe_last_error()
        stream.synchronize()
        for buf, n in ((out, 16), (f32, 8), (ws, need.value)):
            b = buf.cpu().numpy()
            assert (b[:64] == GUARD).all() and (b[64 + n:] == GUARD).all()
        o = out.cpu().numpy()[64:80].view(np.float64)
        n32 = f32.cpu().numpy()[64:68].view(np.float32)[0]
        results.append((p, g, m, v, o.copy(), n32))
    for p, g, m, v, o, n32 in results:
        assert n32 == np.float32(o[0]) == np.float32(want[0]["norm"]) and o[1] == np.float32(MN / (o[0] + 1e-6)) and 0 < o[1] < 1
        for i in range(3):
            assert same(p[i], want[0]["param"][i]) and same(g[i], want[0]["grad"][i]) and same(m[i], want[0]["exp_avg"][i])
            assert same(v[i], want[0]["exp_avg_sq"][i])


# ---------------------------------------------------------------------------------------------- 10
def _steps_on(where, params, groups, grads_per_step, max_norm):
    """the steps of one optimiser over `groups(ps)` on `where`: torch's own clip and step on the CPU, clip_and_step on the device -> (snapshot, ps, opt)"""
    ps = OL.torch_params(params, device=where)
    opt = torch.optim.Adam(groups(ps), lr=OL.LR, eps=OL.EPS)
    for grads in grads_per_step:
        OL.set_grads(ps, grads)
        if where == "cpu":
            norm = torch.nn.utils.clip_grad_norm_(ps, max_norm)
            opt.step()
        else:
            norm = gmpe.clip_and_step(opt, max_norm)
    return OL.snapshot(ps, opt, norm), ps, opt


def _restated(params, grads_per_step, max_norm, **per_tensor):
    r = OL.Restated(params)
    for grads in grads_per_step:
        norm, g = r.step(grads, max_norm, **per_tensor)
    return {"param": r.p, "grad": g, "exp_avg": r.m, "exp_avg_sq": r.v, "norm": norm}, r


def test_a_ninth_hyper_parameter_set_opens_a_launch_group():
    """ten param groups, each with its own lr, eps and weight_decay, in one call: a launch carries eight sets, so the ninth group's tensor opens a second
    launch whose slots 0 and 1 hold the plan's sets 8 and 9"""
    shapes = OL.SHAPES
    n = len(shapes)
    lr, eps, wd = [1e-3 * (i + 1) for i in range(n)], [1e-5 * 3 ** i for i in range(n)], [1e-2 * i for i in range(n)]
    assert n == 10 and OL.MAX_HYPERS == 8
    assert [g[0] for g in OL.geometry([(int(np.prod(s)), OL.IN_NORM | OL.STEP, i) for i, s in enumerate(shapes)])] == [8, 2]
    params = OL.parameters(shapes, seed=10)
    grads = [OL.gradients(shapes, k, 10) for k in range(3)]
    groups = lambda ps: [dict(params=[p], lr=lr[i], eps=eps[i], weight_decay=wd[i]) for i, p in enumerate(ps)]
    truth, _ = _restated(params, grads, OL.MAX_NORM, lr=lr, eps=eps, weight_decay=wd)
    holds(_steps_on(DEV, params, groups, grads, OL.MAX_NORM)[0], _steps_on("cpu", params, groups, grads, OL.MAX_NORM)[0], truth, "ten groups")


def test_a_second_launch_group_whose_first_slot_is_the_plans_second_set():
    """70 tensors in two param groups, the last six in the second: they are the second launch, where the plan's set 1 lies in slot 0"""
    n, cut = 70, OL.MAX_TENSORS
    shapes = ((3,),) * n
    assert [g[0] for g in OL.geometry([(3, OL.IN_NORM | OL.STEP, int(i >= cut)) for i in range(n)])] == [cut, n - cut]
    params = OL.parameters(shapes, seed=11)
    grads = [OL.gradients(shapes, k, 11) for k in range(3)]
    groups = lambda ps: [dict(params=ps[:cut]), dict(params=ps[cut:], lr=3e-3, eps=1e-3, weight_decay=5e-2)]
    per = lambda a, b: [a] * cut + [b] * (n - cut)
    MN = 0.01                                           # under the first tensor's norm alone
    truth, _ = _restated(params, grads, MN, lr=per(OL.LR, 3e-3), eps=per(OL.EPS, 1e-3), weight_decay=per(0.0, 5e-2))
    assert truth["norm"] > MN
    holds(_steps_on(DEV, params, groups, grads, MN)[0], _steps_on("cpu", params, groups, grads, MN)[0], truth, "70 tensors, two groups")


def test_a_tensor_whose_gradient_came_late_has_its_own_step_count_and_bias_correction():
    """one param group; tensor 2 has no gradient in the first two of four steps, so its bias corrections are those of steps 1 and 2 while its
    neighbours' are those of steps 3 and 4"""
    shapes, late = OL.SHAPES[:6], 2
    params = OL.parameters(shapes, seed=12)
    grads = [OL.gradients(shapes, k, 12) for k in range(4)]
    for k in (0, 1):
        grads[k][late] = None
    groups = lambda ps: [dict(params=ps, weight_decay=1e-2)]
    truth, r = _restated(params, grads, OL.MAX_NORM, weight_decay=1e-2)
    assert r.t == [4, 4, 2, 4, 4, 4]
    dev, ps, opt = _steps_on(DEV, params, groups, grads, OL.MAX_NORM)
    ref, _, _ = _steps_on("cpu", params, groups, grads, OL.MAX_NORM)
    assert [float(opt.state[p]["step"]) for p in ps] == [4, 4, 2, 4, 4, 4]
    holds(dev, ref, truth, "a late gradient")
    # with its neighbours' step count the late tensor would be far off: its own was used
    wrong = OL.Restated(params)
    for k in range(4):
        wrong.step(grads[k], OL.MAX_NORM, weight_decay=1e-2)
        wrong.t[late] = k + 1
    assert OL.err(dev["param"][late], wrong.p[late]) > 1e-4
