"""The policy's MLPBase on the device (gmpe.mlp_base, gmpe_mlp_forward / gmpe_mlp_backward) against the reference's own run and the float64 restatement of
tests/mlp_lib.py. err(a) = max|a - a64| / max(1, max|a64|); per array the device is held to err_dev <= 4 * err_ref + 2^-23, err_ref being the error of the
reference's float32 run of the same case (the committed fixture; for the shapes the fixture does not hold, torch's float32 module stack on the CPU, built
here). Everything that is claimed bit for bit is compared bit for bit."""
import ctypes as C
import functools
import os
import types

import numpy as np
import pytest
import torch

import gmpe
import gru_lib as G
import mlp_lib as M
from gmpe import _lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
BIG = (65, (13, 16), 1, "ReLU", 1)


def dev(a, grad=False):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV).requires_grad_(grad)


def make_base(P, case, grad=True, to=dev):
    """a duck-typed MLPBase over the arrays of P -> (base, its parameters in mlp_lib.param_names order)"""
    _, dims, layer_n, act, fnorm = case
    T = {k: to(v, grad) for k, v in P.items()}
    A = type(act, (), {})

    def seq(l):
        return [types.SimpleNamespace(weight=T["w%d" % l], bias=T["b%d" % l]), A(), types.SimpleNamespace(weight=T["lnw%d" % l], bias=T["lnb%d" % l], eps=M.EPS)]
    base = types.SimpleNamespace(_use_feature_normalization=bool(fnorm), mlp=types.SimpleNamespace(fc1=seq(0), fc2=[seq(l) for l in range(1, layer_n + 1)], _layer_N=layer_n))
    if fnorm:
        base.feature_norm = types.SimpleNamespace(weight=T["fn_weight"], bias=T["fn_bias"], eps=M.EPS)
    return base, [T[k] for k in M.param_names(case)]


def run(case, x, gf, P, dims=None, workspace=None):
    """gmpe.mlp_base + torch.autograd.grad of sum(features * gf) -> {name: float32 array} over out_names (of `dims` when the columns are split otherwise)"""
    dims = case[1] if dims is None else dims
    base, ps = make_base(P, case)
    parts = [dev(a, True) for a in M.split(x, dims)]
    f = gmpe.mlp_base(tuple(parts), base, workspace=workspace)
    grads = torch.autograd.grad((f * dev(gf)).sum(), parts + ps)
    torch.cuda.synchronize()
    names = M.out_names((case[0], dims) + case[2:])
    return {k: v.detach().cpu().numpy() for k, v in zip(names, (f,) + tuple(grads))}


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).reshape(-1).view(np.uint32)


def same(a, b):
    return np.asarray(a).shape == np.asarray(b).shape and np.array_equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "mlp_base.npz"))


@functools.lru_cache(maxsize=None)
def truth(case):
    return M.truth64(case)


@functools.lru_cache(maxsize=None)
def device_run(case):
    I, P, _ = truth(case)
    return run(case, I["x"], I["gf"], P)


def torch_stack(P, case):
    """torch's own float32 modules in MLPBase's sequence on the CPU -> (callable on the concatenated input, parameters in param_names order)"""
    _, dims, layer_n, act, fnorm = case
    D = sum(dims)
    mods, ps = [], []
    if fnorm:
        mods.append(torch.nn.LayerNorm(D, eps=M.EPS))
        ps += [mods[-1].weight, mods[-1].bias]
    for l in range(layer_n + 1):
        lin, norm = torch.nn.Linear(D if l == 0 else M.H, M.H), torch.nn.LayerNorm(M.H, eps=M.EPS)
        mods += [lin, torch.nn.ReLU() if act == "ReLU" else torch.nn.Tanh(), norm]
        ps += [lin.weight, lin.bias, norm.weight, norm.bias]
    with torch.no_grad():
        for p, k in zip(ps, M.param_names(case)):
            p.copy_(torch.from_numpy(P[k]))
    return torch.nn.Sequential(*mods), ps


def torch_cpu_reference(case, I, P):
    """-> {name: float32 array}: the source of err_ref where the fixture holds no such shape"""
    net, ps = torch_stack(P, case)
    parts = [torch.from_numpy(a).requires_grad_() for a in M.split(I["x"], case[1])]
    f = net(torch.cat(parts, dim=1))
    grads = torch.autograd.grad((f * torch.from_numpy(I["gf"])).sum(), parts + ps)
    return {k: v.detach().numpy() for k, v in zip(M.out_names(case), (f,) + tuple(grads))}


def check(got, ref32, t64, what, names):
    for k in names:
        e_ref, e_dev = M.err(ref32[k], t64[k]), M.err(got[k], t64[k])
        print("%s %-16s err_ref %.3g err_dev %.3g bound %.3g" % (what, k, e_ref, e_dev, M.bound(e_ref)))
        assert e_ref < M.CAP, (what, k, e_ref)
        assert e_dev <= M.bound(e_ref), (what, k, e_dev, e_ref)


# ---------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("case", M.CASES, ids=M.key)
def test_forward_and_backward_agree_with_the_reference_run(case):
    _, _, t64 = truth(case)
    ref32 = {k: gold()["%s_%s" % (M.key(case), k)] for k in M.out_names(case)}
    check(device_run(case), ref32, t64, M.key(case), M.out_names(case))


@pytest.mark.parametrize("case", [(97, (67,), 2, "ReLU", 1), (40, (7, 130), 0, "Tanh", 1)], ids=M.key)
def test_the_shapes_the_fixture_does_not_hold(case):
    I, P, t64 = truth(case)
    if case[3] == "ReLU":
        assert M.margin(case, M.seed_of(case)) >= M.MARGIN
    check(device_run(case), torch_cpu_reference(case, I, P), t64, M.key(case), M.out_names(case))


# ---------------------------------------------------------------------------------------------- 2
def test_a_row_does_not_depend_on_its_batch():
    I, P, _ = truth(BIG)
    full = device_run(BIG)
    per_row = ["features"] + ["grad_part%d" % i for i in range(len(BIG[1]))]
    a = 0
    for n in (1, 31, 33):                               # the 65 rows as calls of 1, 31 and 33 rows
        got = run((n,) + BIG[1:], I["x"][a:a + n], I["gf"][a:a + n], P)
        for k in per_row:
            assert same(got[k], full[k][a:a + n]), "rows %d .. %d: %s" % (a, a + n - 1, k)
        a += n
    assert a == BIG[0]


def test_the_split_of_the_columns_does_not_show():
    I, P, _ = truth(BIG)
    full = device_run(BIG)
    D = sum(BIG[1])
    one = run(BIG, I["x"], I["gf"], P, dims=(D,))
    assert same(one["features"], full["features"])
    for gp, k in zip(M.split(one["grad_part0"], BIG[1]), ("grad_part0", "grad_part1")):
        assert same(gp, full[k]), k                     # the part gradients are the slices of the concatenated gradient
    for k in ["grad_" + n for n in M.param_names(BIG)]:
        assert same(one[k], full[k]), k
    four = run(BIG, I["x"], I["gf"], P, dims=(1, 12, 15, 1))
    assert same(four["features"], full["features"])
    assert same(np.concatenate([four["grad_part%d" % i] for i in range(4)], 1), one["grad_part0"])
    # a single tensor stands for a 1-tuple
    base, _ = make_base(P, BIG, grad=False)
    assert same(gmpe.mlp_base(dev(I["x"]), base).cpu().numpy(), full["features"])


def test_no_grad_forward_is_the_training_forward_and_takes_no_workspace():
    I, P, _ = truth(BIG)
    full = device_run(BIG)
    base, _ = make_base(P, BIG)                         # parameters that require grad notwithstanding
    parts = tuple(dev(a) for a in M.split(I["x"], BIG[1]))
    with torch.no_grad():
        f = gmpe.mlp_base(parts, base)
        g = gmpe.mlp_base(parts, base, workspace=torch.empty((8,), dtype=torch.uint8, device=DEV))         # a workspace it does not need is not used
    assert not f.requires_grad and f.grad_fn is None and same(f.cpu().numpy(), full["features"]) and same(g.cpu().numpy(), full["features"])
    base, _ = make_base(P, BIG, grad=False)             # nothing requires a gradient: the forward-only plan as well
    f = gmpe.mlp_base(parts, base)
    assert not f.requires_grad and same(f.cpu().numpy(), full["features"])


def test_a_reused_workspace_gives_each_call_the_result_of_a_fresh_one():
    case2 = (BIG[0],) + BIG[1:]
    I, P, _ = truth(BIG)
    J = M.inputs(case2, seed=9)
    full = device_run(BIG)
    other = run(BIG, J["x"], J["gf"], P)
    n = gmpe.mlp_workspace_bytes(BIG[0], sum(BIG[1]), BIG[2])
    ws = torch.full((n + 64,), 0xFF, dtype=torch.uint8, device=DEV)
    a = run(BIG, I["x"], I["gf"], P, workspace=ws)
    b = run(BIG, J["x"], J["gf"], P, workspace=ws)
    c = run(BIG, I["x"], I["gf"], P, workspace=ws)
    for k in M.out_names(BIG):
        assert same(a[k], full[k]) and same(b[k], other[k]) and same(c[k], full[k]), k
    assert bool((ws[n:] == 0xFF).all())                 # nothing is written past gmpe_mlp_workspace_bytes
    with pytest.raises(ValueError, match="workspace must be a contiguous uint8 tensor of at least %d bytes" % n):
        run(BIG, I["x"], I["gf"], P, workspace=ws[:n - 8])


# ---------------------------------------------------------------------------------------------- 3
GUARD = 3                                               # rows behind every output, which the kernels must leave alone


def c_call(case, I, P, backward=True, fill=0, stream=None):
    """gmpe_mlp_forward (+ gmpe_mlp_backward, twice) through ctypes with caller-owned buffers -> {name: array}; fill: the byte the workspace holds before"""
    lib = _lib.load()
    rows, dims, layer_n, act, fnorm = case
    D = sum(dims)
    names = M.param_names(case)
    parts, ps = [dev(a) for a in M.split(I["x"], dims)], [dev(P[k]) for k in names]
    nan = float("nan")
    guarded = lambda r, c: torch.full((r + GUARD, c), nan, device=DEV)
    f = guarded(rows, M.H)
    p = _lib.GmpeMlpPlan()
    p.rows, p.hidden, p.layer_n, p.activation, p.feature_norm, p.n_parts = rows, M.H, layer_n, _lib.MLP_RELU if act == "ReLU" else _lib.MLP_TANH, fnorm, len(dims)
    for i, t in enumerate(parts):
        p.part[i], p.part_dim[i] = t.data_ptr(), dims[i]
    T = dict(zip(names, ps))
    if fnorm:
        p.fn_weight, p.fn_bias, p.fn_eps = T["fn_weight"].data_ptr(), T["fn_bias"].data_ptr(), M.EPS
    for l in range(layer_n + 1):
        p.layer[l].eps = M.EPS
        for k, s in (("weight", "w"), ("bias", "b"), ("ln_weight", "lnw"), ("ln_bias", "lnb")):
            setattr(p.layer[l], k, T["%s%d" % (s, l)].data_ptr())
    p.features = f.data_ptr()
    st = C.c_void_p((stream or torch.cuda.current_stream(torch.device(DEV))).cuda_stream)
    _lib.check(lib.gmpe_mlp_forward(0, C.byref(p), st), "gmpe_mlp_forward")
    outs = [f]
    if backward:
        n = gmpe.mlp_workspace_bytes(rows, D, layer_n)
        ws = torch.full((n + 64,), fill, dtype=torch.uint8, device=DEV)
        gf = dev(I["gf"])
        gparts = [guarded(rows, d) for d in dims]
        gps = [torch.full((t.numel() + GUARD,), nan, device=DEV) for t in ps]
        p.workspace, p.workspace_bytes, p.grad_features, p.features = ws.data_ptr(), n, gf.data_ptr(), None
        for i, t in enumerate(gparts):
            p.grad_part[i] = t.data_ptr()
        G_ = dict(zip(names, gps))
        if fnorm:
            p.grad_fn_weight, p.grad_fn_bias = G_["fn_weight"].data_ptr(), G_["fn_bias"].data_ptr()
        for l in range(layer_n + 1):
            for k, s in (("weight", "w"), ("bias", "b"), ("ln_weight", "lnw"), ("ln_bias", "lnb")):
                setattr(p.layer[l], "grad_" + k, G_["%s%d" % (s, l)].data_ptr())
        for rep in range(2):                            # backward may be repeated on one plan: fresh outputs, the same bits
            _lib.check(lib.gmpe_mlp_backward(0, C.byref(p), st), "gmpe_mlp_backward")
            if rep == 0:
                torch.cuda.synchronize()
                first = [g.clone() for g in gparts + gps]
                for g in gparts + gps:
                    g.fill_(nan)
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        for a, b in zip(first, gparts + gps):
            assert same(a.cpu().numpy(), b.cpu().numpy()), "the second backward call differs"
        assert bool((ws[n:] == fill).all())
        outs += gparts + gps
    torch.cuda.synchronize()
    res = {}
    for k, t, like in zip(M.out_names(case), outs, [None] * (1 + len(dims)) + ps if backward else [None]):
        a = t.cpu().numpy()
        if like is None:
            assert np.isnan(a[rows:]).all(), "rows past the end of %s were written" % k
            res[k] = a[:rows]
        else:
            assert np.isnan(a[like.numel():]).all(), "elements past the end of %s were written" % k
            res[k] = a[:like.numel()].reshape(tuple(like.shape))
    return res


@pytest.mark.parametrize("case", [BIG, (65, (256,), 2, "ReLU", 1), (33, (15, 16, 4), 1, "Tanh", 1), (65, (15, 16), 2, "Tanh", 0), (2, (2,), 1, "ReLU", 1)], ids=M.key)
def test_the_c_entries_give_the_wrappers_bits_and_stay_inside_their_outputs(case):
    I, P, _ = truth(case)
    a, b = device_run(case), c_call(case, I, P)
    for k in M.out_names(case):
        assert same(a[k], b[k]), k


def test_the_workspaces_old_contents_do_not_show_and_a_side_stream_works():
    I, P, _ = truth(BIG)
    full = device_run(BIG)
    ones = c_call(BIG, I, P, fill=0xFF)
    fwd = c_call(BIG, I, P, backward=False)
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        other = c_call(BIG, I, P, stream=side)
        wrapped = run(BIG, I["x"], I["gf"], P)          # the wrapper launches on the current stream
    for k in M.out_names(BIG):
        assert same(ones[k], full[k]) and same(other[k], full[k]) and same(wrapped[k], full[k]), k
    assert same(fwd["features"], full["features"])


# ---------------------------------------------------------------------------------------------- 4
def test_mlp_base_chained_into_rnn_layer():
    """gradients reach the parts and both modules' parameters through the two nodes; against the CPU torch chain (MLPBase-shaped stack, step-by-step GRU,
    LayerNorm) under the same rule, at 10 steps x 7 rows"""
    L, Nb = 10, 7
    case = (L * Nb, (13, 16), 1, "ReLU", 1)
    I, P, _ = truth(case)
    GP, GI, m = G.params(3), G.inputs(L, Nb, 3), G.masks(L, Nb, "random", 3)
    # device
    base, ps = make_base(P, case)
    rnn = types.SimpleNamespace(weight_ih_l0=dev(GP["weight_ih"], True), weight_hh_l0=dev(GP["weight_hh"], True), bias_ih_l0=dev(GP["bias_ih"], True),
                                bias_hh_l0=dev(GP["bias_hh"], True))
    layer = types.SimpleNamespace(rnn=rnn, norm=types.SimpleNamespace(weight=dev(GP["ln_weight"], True), bias=dev(GP["ln_bias"], True), eps=G.EPS), _recurrent_N=1)
    gps = [rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0, layer.norm.weight, layer.norm.bias]
    parts, hxs = [dev(a, True) for a in M.split(I["x"], case[1])], dev(GI["hxs"], True)
    f, ho = gmpe.rnn_layer(gmpe.mlp_base(tuple(parts), base), hxs, dev(m), layer)
    leaves = parts + [hxs] + ps + gps
    grads = torch.autograd.grad((f * dev(GI["gf"])).sum() + (ho * dev(GI["gh"])).sum(), leaves)
    torch.cuda.synchronize()
    names = ["features", "hxs_out"] + ["grad_part0", "grad_part1", "grad_hxs"] + ["grad_" + k for k in M.param_names(case)] + ["grad_" + k for k in G.PARAMS]
    got = {k: v.detach().cpu().numpy() for k, v in zip(names, (f, ho) + tuple(grads))}
    # the CPU torch chain, float32
    net, tps = torch_stack(P, case)
    gru, norm = torch.nn.GRU(G.D, G.H), torch.nn.LayerNorm(G.H, eps=G.EPS)
    tg = [gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0, norm.weight, norm.bias]
    with torch.no_grad():
        for p, k in zip(tg, G.PARAMS):
            p.copy_(torch.from_numpy(GP[k]))
    tparts, thxs = [torch.from_numpy(a).requires_grad_() for a in M.split(I["x"], case[1])], torch.from_numpy(GI["hxs"]).requires_grad_()
    x = net(torch.cat(tparts, dim=1))
    mt, h, outs = torch.from_numpy(m).view(L, 1, Nb, 1), thxs.transpose(0, 1), []
    for t in range(L):
        o, h = gru(x.view(L, Nb, G.D)[t:t + 1], h * mt[t])
        outs.append(o)
    tf, tho = norm(torch.cat(outs).reshape(L * Nb, G.H)), h.transpose(0, 1)
    tgrads = torch.autograd.grad((tf * torch.from_numpy(GI["gf"])).sum() + (tho * torch.from_numpy(GI["gh"])).sum(), tparts + [thxs] + tps + tg)
    ref32 = {k: v.detach().numpy() for k, v in zip(names, (tf, tho) + tuple(tgrads))}
    # the float64 truth: the GRU's restatement on the MLP's, and back
    x64 = M.forward64(I["x"], P, case)
    f64, h64 = G.forward64(x64, GI["hxs"], m, GP)
    g64 = G.backward64(x64, GI["hxs"], m, GP, GI["gf"], GI["gh"])
    b64 = M.backward64(I["x"], P, g64["grad_x"], case)
    t64 = dict(features=f64, hxs_out=h64, grad_hxs=g64["grad_hxs"])
    t64.update({"grad_part%d" % i: a for i, a in enumerate(M.split(b64.pop("grad_x"), case[1]))})
    t64.update(b64)
    t64.update({k: g64[k] for k in ["grad_" + n for n in G.PARAMS]})
    assert sorted(t64) == sorted(names)
    check(got, ref32, t64, "mlp_base -> rnn_layer", names)
