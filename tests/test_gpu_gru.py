"""The masked GRU layer on the device (gmpe.rnn_layer, gmpe_gru_forward / gmpe_gru_backward) against the reference's own run and the float64 restatement
of tests/gru_lib.py. err(a) = max|a - a64| / max(1, max|a64|); per array the device is held to err_dev <= 4 * err_ref + 2^-23, err_ref being the error of
the reference's float32 run of the same case (the committed fixture; for the shapes the fixture does not hold, torch's float32 nn.GRU + nn.LayerNorm on
the CPU, driven step by step here). Everything that is claimed bit for bit is compared bit for bit."""
import ctypes as C
import functools
import os
import types

import numpy as np
import pytest
import torch

import gmpe
import gru_lib as G
from gmpe import _lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
OUT = ("features", "hxs_out") + G.GRADS


def dev(a, grad=False):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV).requires_grad_(grad)


def make_layer(P, grad=True):
    rnn = types.SimpleNamespace(weight_ih_l0=dev(P["weight_ih"], grad), weight_hh_l0=dev(P["weight_hh"], grad), bias_ih_l0=dev(P["bias_ih"], grad),
                                bias_hh_l0=dev(P["bias_hh"], grad))
    norm = types.SimpleNamespace(weight=dev(P["ln_weight"], grad), bias=dev(P["ln_bias"], grad), eps=G.EPS)
    return types.SimpleNamespace(rnn=rnn, norm=norm, _recurrent_N=1)


def layer_params(layer):
    return [layer.rnn.weight_ih_l0, layer.rnn.weight_hh_l0, layer.rnn.bias_ih_l0, layer.rnn.bias_hh_l0, layer.norm.weight, layer.norm.bias]


def run(I, m, P, gf=None, gh=None, workspace=None):
    """gmpe.rnn_layer + torch.autograd.grad of sum(features * gf) + sum(hxs_out * gh) -> {name: float32 array} over OUT"""
    layer = make_layer(P)
    x, hxs = dev(I["x"], True), dev(I["hxs"], True)
    f, h = gmpe.rnn_layer(x, hxs, dev(m), layer, workspace=workspace)
    loss = (f * dev(I["gf"] if gf is None else gf)).sum() + (h * dev(I["gh"] if gh is None else gh)).sum()
    grads = torch.autograd.grad(loss, [x, hxs] + layer_params(layer))
    torch.cuda.synchronize()
    return {k: v.detach().cpu().numpy() for k, v in zip(OUT, (f, h) + tuple(grads))}


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).reshape(-1).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def gold(pattern):
    return np.load(os.path.join(ROOT, "tests", "golden", "gru_layer_%s.npz" % pattern))


@functools.lru_cache(maxsize=None)
def truth(L, Nb, pattern, seed=0):
    return G.truth64(L, Nb, pattern, seed)


def torch_cpu_reference(I, m, P):
    """torch's float32 nn.GRU + nn.LayerNorm on the CPU, one step at a time with the state times the step's mask (equal to the segment loop for 0 / 1
    masks), and autograd -> {name: float32 array}: the source of err_ref where the fixture holds no such shape"""
    Nb = I["hxs"].shape[0]
    L = I["x"].shape[0] // Nb
    gru, norm = torch.nn.GRU(G.D, G.H), torch.nn.LayerNorm(G.H, eps=G.EPS)
    ps = [gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0, norm.weight, norm.bias]
    with torch.no_grad():
        for p, k in zip(ps, G.PARAMS):
            p.copy_(torch.from_numpy(P[k]))
    x, hxs = torch.from_numpy(I["x"]).requires_grad_(), torch.from_numpy(I["hxs"]).requires_grad_()
    mt, h, outs = torch.from_numpy(m).view(L, 1, Nb, 1), hxs.transpose(0, 1), []
    for t in range(L):
        o, h = gru(x.view(L, Nb, G.D)[t:t + 1], h * mt[t])
        outs.append(o)
    f, ho = norm(torch.cat(outs).reshape(L * Nb, G.H)), h.transpose(0, 1)
    loss = (f * torch.from_numpy(I["gf"])).sum() + (ho * torch.from_numpy(I["gh"])).sum()
    grads = torch.autograd.grad(loss, [x, hxs] + ps)
    return {k: v.detach().numpy() for k, v in zip(OUT, (f, ho) + tuple(grads))}


def check(got, ref32, t64, what, names=OUT):
    for k in names:
        e_ref, e_dev = G.err(ref32[k], t64[k]), G.err(got[k], t64[k])
        print("%s %-16s err_ref %.3g err_dev %.3g bound %.3g" % (what, k, e_ref, e_dev, G.bound(e_ref)))
        assert e_ref < G.CAP, (what, k, e_ref)
        assert e_dev <= G.bound(e_ref), (what, k, e_dev, e_ref)


# ---------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("L,Nb", G.CASES)
@pytest.mark.parametrize("pattern", G.PATTERNS)
def test_forward_and_backward_agree_with_the_reference_run(L, Nb, pattern):
    I, m, P, t64 = truth(L, Nb, pattern)
    d = gold(pattern)
    ref32 = {k: d["%s_%s" % (G.key(L, Nb, pattern), k)] for k in OUT}
    check(run(I, m, P), ref32, t64, G.key(L, Nb, pattern))


@pytest.mark.parametrize("L,Nb", [(1, 1), (25, 2)])
def test_the_shapes_the_fixture_does_not_hold(L, Nb):
    for pattern in ("ones", "random"):
        I, m, P, t64 = truth(L, Nb, pattern)
        check(run(I, m, P), torch_cpu_reference(I, m, P), t64, G.key(L, Nb, pattern))


# ---------------------------------------------------------------------------------------------- 2
GUARD = 3                                               # rows behind every output, which the kernels must leave alone


def c_call(I, m, P, backward=True, fill=None, gh=True):
    """gmpe_gru_forward (+ gmpe_gru_backward) through ctypes -> {name: array}; fill: the byte the workspace holds before forward. Every output has GUARD
    rows of NaN behind it and the workspace 64 bytes of `fill`, which must be intact afterwards."""
    lib = _lib.load()
    Nb = I["hxs"].shape[0]
    L = I["x"].shape[0] // Nb
    ins = [dev(I["x"]), dev(I["hxs"]), dev(m)] + [dev(P[k]) for k in G.PARAMS]
    nan = float("nan")
    guarded = lambda shape: torch.full((shape[0] + GUARD,) + tuple(shape[1:]), nan, device=DEV)
    f, ho = guarded((L * Nb, G.H)), guarded((Nb, 1, G.H))
    p = _lib.GmpeGruPlan()
    p.steps, p.rows, p.in_dim, p.hidden, p.eps = L, Nb, G.D, G.H, G.EPS
    for k, t in zip(("x", "hxs", "masks") + G.PARAMS, ins):
        setattr(p, k, t.data_ptr())
    p.features, p.hxs_out = f.data_ptr(), ho.data_ptr()
    ws = None
    if backward:
        n = gmpe.rnn_workspace_bytes(L, Nb, G.H)
        fill = 0 if fill is None else fill
        ws = torch.full((n + 64,), fill, dtype=torch.uint8, device=DEV)
        p.workspace, p.workspace_bytes = ws.data_ptr(), n
    st = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    _lib.check(lib.gmpe_gru_forward(0, C.byref(p), st), "gmpe_gru_forward")
    out, like = [f, ho], [(L * Nb, G.H), (Nb, 1, G.H)]
    if backward:
        gf, ghx = dev(I["gf"]), dev(I["gh"])
        grads = [guarded(t.shape) for t in ins[:2] + ins[3:]]
        like += [tuple(t.shape) for t in ins[:2] + ins[3:]]
        p.grad_features = gf.data_ptr()
        p.grad_hxs_out = ghx.data_ptr() if gh else None
        for k, t in zip(G.GRADS, grads):
            setattr(p, k, t.data_ptr())
        for rep in range(2):                            # backward may be repeated on one forward's workspace: fresh outputs, the same bits
            _lib.check(lib.gmpe_gru_backward(0, C.byref(p), st), "gmpe_gru_backward")
            if rep == 0:
                first = [g.clone() for g in grads]
                for g in grads:
                    g.fill_(float("nan"))
        torch.cuda.synchronize()
        for a, b, k in zip(first, grads, G.GRADS):
            assert same(a.cpu().numpy(), b.cpu().numpy()), "the second backward call differs: " + k
        assert bool((ws[n:] == fill).all()), "bytes past gmpe_gru_workspace_bytes were written"
        out += grads
    torch.cuda.synchronize()
    res = {}
    for k, t, shape in zip(OUT, out, like):
        a = t.cpu().numpy()
        assert np.isnan(a[shape[0]:]).all(), "rows past the end of %s were written" % k
        res[k] = a[:shape[0]]
    return res


@pytest.mark.parametrize("L,Nb", [(2, 3), (10, 2 * G.TILE + 1)])
def test_the_c_entries_give_the_wrappers_bits(L, Nb):
    I, m, P, _ = truth(L, Nb, "random")
    a, b = run(I, m, P), c_call(I, m, P)
    for k in OUT:
        assert same(a[k], b[k]), k
    # grad_hxs_out == NULL stands for zeros
    z = run(I, m, P, gh=np.zeros_like(I["gh"]))
    n = c_call(I, m, P, gh=False)
    for k in OUT:
        assert same(z[k], n[k]), k


# ---------------------------------------------------------------------------------------------- 3
def test_one_call_over_L_steps_is_L_calls_over_one_step():
    L, Nb = 10, G.TILE + 3
    I, m, P, _ = truth(L, Nb, "random", seed=1)
    layer = make_layer(P, grad=False)
    with torch.no_grad():
        f, h = gmpe.rnn_layer(dev(I["x"]), dev(I["hxs"]), dev(m), layer)
        hs, x3, m3 = dev(I["hxs"]), dev(I["x"]).view(L, Nb, G.D), dev(m).view(L, Nb, 1)
        for t in range(L):
            ft, hs = gmpe.rnn_layer(x3[t], hs, m3[t], layer)
            assert torch.equal(ft.view(torch.int32), f.view(L, Nb, G.H)[t].view(torch.int32)), t
        assert torch.equal(hs.view(torch.int32), h.view(torch.int32))


# ---------------------------------------------------------------------------------------------- 4
def test_a_row_does_not_depend_on_its_batch():
    L, Nb = 10, 2 * G.TILE + 1
    I, m, P, t64 = truth(L, Nb, "random")
    full = run(I, m, P)
    rows3 = lambda a, n: np.asarray(a).reshape(-1, n, a.shape[-1])                  # [L or 1, n, cols]
    per_row = ("features", "hxs_out", "grad_x", "grad_hxs")
    cut = {k: rows3(full[k], Nb) if k in ("features", "grad_x") else full[k].reshape(1, Nb, G.H) for k in per_row}

    def subset(idx):
        sel = lambda a: np.ascontiguousarray(rows3(a, Nb)[:, idx]).reshape(-1, a.shape[-1])
        J = dict(x=sel(I["x"]), hxs=np.ascontiguousarray(I["hxs"][idx]), gf=sel(I["gf"]), gh=np.ascontiguousarray(I["gh"][idx]))
        return run(J, sel(m), P)
    perm = np.random.RandomState(4).permutation(Nb)
    got = subset(perm)
    for k in per_row:
        g = rows3(got[k], Nb) if k in ("features", "grad_x") else got[k].reshape(1, Nb, G.H)
        assert same(g, cut[k][:, perm]), "permuted batch: " + k
    ref32 = {k: gold("random")["%s_%s" % (G.key(L, Nb, "random"), k)] for k in OUT}
    check(got, ref32, t64, "permuted batch", names=tuple("grad_" + k for k in G.PARAMS))          # another summation order: the tolerance only
    for r in (0, G.TILE - 1, G.TILE, Nb - 1):                                                       # alone: tile 0's first lane row, both sides of a tile edge, the tail
        one = subset(np.array([r]))
        for k in per_row:
            g = rows3(one[k], 1) if k in ("features", "grad_x") else one[k].reshape(1, 1, G.H)
            assert same(g, cut[k][:, [r]]), "row %d alone: %s" % (r, k)


# ---------------------------------------------------------------------------------------------- 5
def test_a_zero_mask_cuts_the_state_and_the_gradient():
    L, Nb = 10, G.TILE + 5
    I, m, P, _ = truth(L, Nb, "random", seed=2)
    m2 = m.reshape(L, Nb).copy()
    base = run(I, m, P)
    start0 = np.flatnonzero(m2[0] == 0)
    assert 0 < len(start0) < Nb
    # rows whose first mask is 0 never see their incoming state
    J = dict(I)
    J["hxs"] = I["hxs"].copy()
    J["hxs"][start0] = 1e30
    huge = run(J, m, P)
    for k in OUT:
        assert same(base[k], huge[k]), k
    assert (base["grad_hxs"][start0] == 0).all() and np.abs(base["grad_hxs"][np.flatnonzero(m2[0] == 1)]).max() > 0
    # a zero at step t of row k: nothing flows from the outputs of steps >= t to that row's x before t
    gx = base["grad_x"].reshape(L, Nb, G.D)
    checked = 0
    for k in range(Nb):
        ts = np.flatnonzero(m2[1:, k] == 0) + 1
        if len(ts) == 0:
            continue
        t = int(ts[0])
        gf = I["gf"].reshape(L, Nb, G.H).copy()
        gf[t:, k] += 1.0
        gh = I["gh"].copy()
        gh[k] -= 2.0
        pert = run(I, m, P, gf=gf.reshape(L * Nb, G.H), gh=gh)["grad_x"].reshape(L, Nb, G.D)
        assert same(pert[:t, k], gx[:t, k]) and not same(pert[t:, k], gx[t:, k]), (k, t)
        checked += 1
        if checked == 3:
            break
    assert checked == 3


# ---------------------------------------------------------------------------------------------- 6
def test_determinism_and_the_two_plans():
    L, Nb = 10, 2 * G.TILE + 1
    I, m, P, _ = truth(L, Nb, "random")
    zero, ones = c_call(I, m, P, fill=0), c_call(I, m, P, fill=0xFF)            # c_call itself calls backward twice into fresh outputs
    for k in OUT:
        assert same(zero[k], ones[k]), "the workspace's old contents show in " + k
    fwd = c_call(I, m, P, backward=False)
    for k in ("features", "hxs_out"):
        assert same(fwd[k], zero[k]), "forward-only plan: " + k
    layer = make_layer(P)
    with torch.no_grad():                               # the wrapper's forward-only path, parameters that require grad notwithstanding
        f, h = gmpe.rnn_layer(dev(I["x"]), dev(I["hxs"]), dev(m), layer)
    assert not f.requires_grad and same(f.cpu().numpy(), zero["features"]) and same(h.cpu().numpy(), zero["hxs_out"])
    # hxs_out may be hxs itself in a forward-only plan: the rollout's in-place state update
    lib = _lib.load()
    ins = [dev(I["x"]), dev(I["hxs"]), dev(m)] + [dev(P[k]) for k in G.PARAMS]
    f2 = torch.empty((L * Nb, G.H), device=DEV)
    p = _lib.GmpeGruPlan()
    p.steps, p.rows, p.in_dim, p.hidden, p.eps = L, Nb, G.D, G.H, G.EPS
    for k, t in zip(("x", "hxs", "masks") + G.PARAMS, ins):
        setattr(p, k, t.data_ptr())
    p.features, p.hxs_out = f2.data_ptr(), ins[1].data_ptr()
    _lib.check(lib.gmpe_gru_forward(0, C.byref(p), C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)), "gmpe_gru_forward")
    torch.cuda.synchronize()
    assert same(f2.cpu().numpy(), zero["features"]) and same(ins[1].cpu().numpy(), zero["hxs_out"])


def test_the_calls_can_be_captured_in_a_graph():
    """no allocation, no host synchronisation inside the C entries: forward and backward replay from a captured graph with the eager bits"""
    L, Nb = 3, G.TILE + 1
    I, m, P, _ = truth(L, Nb, "random", seed=3)
    eager = c_call(I, m, P)                             # also raises the kernels' dynamic LDS limits before the capture
    lib = _lib.load()
    ins = [dev(I["x"]), dev(I["hxs"]), dev(m)] + [dev(P[k]) for k in G.PARAMS]
    f, ho, gf, gh = torch.empty((L * Nb, G.H), device=DEV), torch.empty((Nb, 1, G.H), device=DEV), dev(I["gf"]), dev(I["gh"])
    grads = [torch.empty_like(t) for t in ins[:2] + ins[3:]]
    ws = torch.empty((gmpe.rnn_workspace_bytes(L, Nb, G.H),), dtype=torch.uint8, device=DEV)
    p = _lib.GmpeGruPlan()
    p.steps, p.rows, p.in_dim, p.hidden, p.eps = L, Nb, G.D, G.H, G.EPS
    for k, t in zip(("x", "hxs", "masks") + G.PARAMS + ("features", "hxs_out", "grad_features", "grad_hxs_out") + G.GRADS, ins + [f, ho, gf, gh] + grads):
        setattr(p, k, t.data_ptr())
    p.workspace, p.workspace_bytes = ws.data_ptr(), ws.numel()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                       # one stream, a linear chain of four launches: no parallel branches
        st = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
        _lib.check(lib.gmpe_gru_forward(0, C.byref(p), st), "gmpe_gru_forward")
        _lib.check(lib.gmpe_gru_backward(0, C.byref(p), st), "gmpe_gru_backward")
    for t in [f, ho] + grads:
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for k, t in zip(OUT, [f, ho] + grads):
        assert same(t.cpu().numpy(), eager[k]), k


# ---------------------------------------------------------------------------------------------- 7
def test_the_buffers_recurrent_minibatch_is_in_the_layers_row_order():
    """rnn_states and masks as DeviceRolloutBuffer.recurrent_generator yields them, fed to gmpe.rnn_layer with a seeded x: every chunk k on its own,
    restated sequentially from rows l * chunks + k, gives the layer's rows."""
    from gmpe.engine import GmpeEngine
    from gmpe.minibatch import TUPLE
    from gmpe.rollout import DeviceRolloutBuffer
    N, A, T, L = 4, 3, 10, 5
    cfg = gmpe.make_config(num_envs=N, num_agents=A, episode_length=4, seed=6)
    eng = GmpeEngine(cfg, device=0)
    buf = DeviceRolloutBuffer(eng, T, policy_fields="all", learner_fields="all", recurrent_N=1, hidden_size=G.H)
    buf.warmup()
    g = torch.Generator(device=eng.device)
    g.manual_seed(11)
    for t in range(T):
        action = torch.randint(0, cfg.n_actions, (N * A, 1), generator=g, device=eng.device)
        buf.insert_step(action.view(N, A).to(torch.int32), values=torch.randn((N * A, 1), generator=g, device=eng.device), actions=action,
                        action_log_probs=torch.randn((N * A, 1), generator=g, device=eng.device),
                        rnn_states=torch.rand((N * A, 1, G.H), generator=g, device=eng.device) * 2 - 1,
                        rnn_states_critic=torch.rand((N * A, 1, G.H), generator=g, device=eng.device) * 2 - 1)
    adv = torch.randn((T, N, A, 1), generator=g, device=eng.device)
    mb = next(iter(buf.recurrent_generator(adv, 1, L)))
    hxs, masks = mb[TUPLE.index("rnn_states")], mb[TUPLE.index("masks")]
    chunks = T * N * A // L
    assert tuple(hxs.shape) == (chunks, 1, G.H) and tuple(masks.shape) == (L * chunks, 1)
    mk = masks.cpu().numpy()
    assert set(np.unique(mk)) == {0.0, 1.0}                                  # episodes of 4 steps: some chunks hold a reset
    P, I = G.params(7), G.inputs(L, chunks, 7)
    I["hxs"] = hxs.cpu().numpy()
    got = run(I, mk, P)
    f64 = np.empty((L, chunks, G.H))
    h64 = np.empty((chunks, 1, G.H))
    x3, m3 = I["x"].reshape(L, chunks, G.D), mk.reshape(L, chunks, 1)
    for k in range(chunks):                                                  # one chunk at a time, one step at a time
        h = I["hxs"][k:k + 1]
        for l in range(L):
            fl, h = G.forward64(x3[l, k:k + 1], h, m3[l, k:k + 1], P)
            f64[l, k] = fl[0]
        h64[k] = h[0]
    ref32 = torch_cpu_reference(I, mk, P)
    check(got, ref32, dict(features=f64.reshape(L * chunks, G.H), hxs_out=h64), "buffer minibatch", names=("features", "hxs_out"))
    eng.check_errors()
    eng.close()
