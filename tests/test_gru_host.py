"""Host side of the masked GRU layer (include/gmpe.h gmpe_gru_forward / gmpe_gru_backward, gmpe.rnn_layer), no GPU:
(a) the two float64 restatements of tests/gru_lib.py (per-row masking, the reference's segment loop) are bit-identical, and agree with the reference's
    own float32 run (tests/golden/gru_layer_<pattern>.npz, made by tests/golden/make_gru_fixture.py) under the project's parity bar, 1e-5, per array;
(b) the exported symbols, the plan's layout against the C header, and the refusals of both layers, which need no device;
(c) the compiler's resource report of csrc/gmpe_gru.hip shows no scratch memory."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import abi_lib
import gmpe
import gru_lib as G
from gmpe import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = [(L, Nb, pat) for L, Nb in G.CASES for pat in G.PATTERNS]


def gold(pattern):
    return np.load(os.path.join(ROOT, "tests", "golden", "gru_layer_%s.npz" % pattern))


# ---------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("L,Nb,pattern", ALL)
def test_the_two_restatements_are_bit_identical(L, Nb, pattern):
    P, I, m = G.params(), G.inputs(L, Nb), G.masks(L, Nb, pattern)
    f1, h1 = G.forward64(I["x"], I["hxs"], m, P)
    f2, h2 = G.segment64(I["x"], I["hxs"], m, P)
    assert f1.dtype == np.float64 and np.array_equal(f1, f2) and np.array_equal(h1, h2)


def test_the_mask_patterns_hold_what_the_fixture_promises():
    assert G.TILE == _lib.GRU_ROW_TILE and G.CASES[-1] == (10, 2 * G.TILE + 1)
    for L, Nb in G.CASES:
        m = G.masks(L, Nb, "random").reshape(L, Nb)
        assert set(np.unique(m)) <= {0.0, 1.0} and (m[:, Nb - 1] == 0).all()
        if Nb > 1:
            assert (m[:L - 1, 0] == 1).all() and m[L - 1, 0] == 0
        m = G.masks(L, Nb, "row0_t0").reshape(L, Nb)
        assert m[0, 0] == 0 and m.sum() == L * Nb - 1
        assert G.masks(L, Nb, "ones").all() and not G.masks(L, Nb, "zeros").any()


@pytest.mark.parametrize("pattern", G.PATTERNS)
def test_the_restatement_agrees_with_the_reference_run_under_the_cap(pattern):
    d = gold(pattern)
    for L, Nb in G.CASES:
        _, _, _, t = G.truth64(L, Nb, pattern)
        for k, v in t.items():
            ref = d["%s_%s" % (G.key(L, Nb, pattern), k)]
            assert ref.dtype == np.float32 and ref.shape == v.shape, k
            e = G.err(ref, v)
            print("%s %-16s err_ref %.3g" % (G.key(L, Nb, pattern), k, e))
            assert e < G.CAP, (L, Nb, pattern, k, e)


def test_backward64_is_the_derivative_of_forward64():
    """the hand-written float64 backward against central differences of the float64 forward, on a few coordinates of every input"""
    L, Nb = 3, 2
    P, I, m = G.params(5), G.inputs(L, Nb, 5), G.masks(L, Nb, "row0_t0")
    m[2 * Nb + 1] = 0
    g = G.backward64(I["x"], I["hxs"], m, P, I["gf"], I["gh"])

    def loss(x, hxs, P):
        f, h = G.forward64(x, hxs, m, P)
        return (f * I["gf"]).sum() + (h * I["gh"]).sum()
    rng = np.random.RandomState(0)
    x64, h64, P64 = I["x"].astype(np.float64), I["hxs"].astype(np.float64), {k: v.astype(np.float64) for k, v in P.items()}
    for name in G.GRADS:
        arr = x64 if name == "grad_x" else h64 if name == "grad_hxs" else P64[name[5:]]
        for _ in range(4):
            i = tuple(rng.randint(0, s) for s in arr.shape)
            old, hstep = arr[i], 1e-6
            arr[i] = old + hstep
            up = loss(x64, h64, P64)
            arr[i] = old - hstep
            dn = loss(x64, h64, P64)
            arr[i] = old
            num = (up - dn) / (2 * hstep)
            assert abs(num - g[name][i]) <= 1e-6 * max(1.0, abs(num)), (name, i, num, g[name][i])


# ---------------------------------------------------------------------------------------------- (b)
def test_symbols_are_exported_and_the_plan_matches_the_header():
    lib = _lib.load()
    assert {"gmpe_gru_workspace_bytes", "gmpe_gru_forward", "gmpe_gru_backward"} <= set(_lib.SYMBOLS) & abi_lib.exported()
    assert lib.gmpe_abi_version() == 3 and gmpe.config.ABI_VERSION == 3 == abi_lib.constant("GMPE_ABI_VERSION")   # added entry points: the ABI version stays
    PP = _lib.GmpeGruPlan
    assert abi_lib.layout(PP) == abi_lib.mirror_layout(PP) and C.sizeof(PP) == 2 * 8 + 2 * 4 + 8 + 22 * 8 + 8
    assert abi_lib.constant("GMPE_GRU_ROW_TILE") == _lib.GRU_ROW_TILE


def test_workspace_bytes():
    lib = _lib.load()
    n = C.c_size_t(7)
    assert lib.gmpe_gru_workspace_bytes(10, 100, 64, 0, C.byref(n)) == 0 and n.value == 0          # the forward-only plan takes none
    assert lib.gmpe_gru_workspace_bytes(10, 100, 64, 1, C.byref(n)) == 0
    # gates, the W_hn h + b_hn term, the h sequence, the LayerNorm statistics, and as much again for the gate gradients
    assert n.value >= 1000 * (4 * 64 + 64 + 2) * 4 and n.value % 8 == 0
    assert gmpe.rnn_workspace_bytes(10, 100, 64) == n.value and gmpe.rnn_workspace_bytes(10, 100, 64, backward=False) == 0
    for args, field in (((0, 5, 64, 1), "steps"), ((5, 0, 64, 1), "rows"), ((5, 5, 32, 1), "hidden"), ((5, 5, 64, 2), "want_backward")):
        assert lib.gmpe_gru_workspace_bytes(*args, C.byref(n)) == -1
        assert field in lib.gmpe_last_error().decode()
    assert lib.gmpe_gru_workspace_bytes(5, 5, 64, 1, None) == -1 and "bytes_out" in lib.gmpe_last_error().decode()
    with pytest.raises(NotImplementedError, match="hidden = 32"):
        gmpe.rnn_workspace_bytes(10, 100, 32)


INPUTS = ("x", "hxs", "masks", "weight_ih", "weight_hh", "bias_ih", "bias_hh", "ln_weight", "ln_bias")
FWD_ONLY = ("features", "hxs_out")
BWD_ONLY = ("grad_features", "grad_x", "grad_hxs", "grad_weight_ih", "grad_weight_hh", "grad_bias_ih", "grad_bias_hh", "grad_ln_weight", "grad_ln_bias")
MB = 1 << 20


def _plan(**over):
    """a plan over fake, well separated addresses (1 MiB apart): nothing here reaches a device"""
    p = _lib.GmpeGruPlan()
    p.steps, p.rows, p.in_dim, p.hidden, p.eps = 4, 10, 64, 64, 1e-5
    for i, k in enumerate(INPUTS + FWD_ONLY + BWD_ONLY + ("grad_hxs_out", "workspace")):
        setattr(p, k, (i + 1) * MB)
    p.workspace_bytes = MB
    for k, v in over.items():
        setattr(p, k, v)
    return p


def _refused(fn, plan, *names):
    lib = _lib.load()
    assert getattr(lib, fn)(0, C.byref(plan), None) == -1
    msg = lib.gmpe_last_error().decode()
    assert msg.startswith(fn + ":") and all(n in msg for n in names), msg
    return msg


@pytest.mark.parametrize("fn", ["gmpe_gru_forward", "gmpe_gru_backward"])
def test_c_entry_points_refuse_bad_plans_before_any_device_call(fn):
    lib = _lib.load()
    assert getattr(lib, fn)(0, None, None) == -1 and "null plan" in lib.gmpe_last_error().decode()
    for bad, name in ((dict(steps=0), "steps"), (dict(steps=-3), "steps"), (dict(rows=0), "rows"), (dict(in_dim=32), "in_dim"), (dict(hidden=128), "hidden"),
                      (dict(in_dim=0, hidden=0), "in_dim"), (dict(eps=0.0), "eps"), (dict(eps=float("nan")), "eps"), (dict(workspace_bytes=64), "workspace_bytes"),
                      (dict(workspace=23 * MB + 4), "workspace"), (dict(x=MB + 2), "x"), (dict(steps=1 << 41), "steps")):
        _refused(fn, _plan(**bad), name)
    needed = INPUTS + (FWD_ONLY if fn == "gmpe_gru_forward" else BWD_ONLY + ("workspace",))
    for k in needed:
        _refused(fn, _plan(**{k: None}), k)


def test_what_each_entry_point_does_not_need_may_be_null():
    """a forward-only plan: no gradient pointers, no workspace; a backward plan: no features, no hxs_out, no grad_hxs_out. The plans pass the host's checks
    and fail at the first device call (there is none here), or succeed in reaching it: either way the error is not an argument error."""
    lib = _lib.load()
    for fn, nulls in (("gmpe_gru_forward", BWD_ONLY + ("grad_hxs_out", "workspace")), ("gmpe_gru_backward", FWD_ONLY + ("grad_hxs_out",))):
        p = _plan(**{k: None for k in nulls})
        if "workspace" in nulls:
            p.workspace_bytes = 0
        if torch.cuda.is_available():
            continue                                    # fake addresses must not reach a real device
        assert getattr(lib, fn)(0, C.byref(p), None) == -2, lib.gmpe_last_error().decode()          # GMPE_ERR_HIP: every host check passed


def test_hxs_out_may_alias_hxs_in_a_forward_only_plan_and_nothing_else():
    fn = "gmpe_gru_forward"
    for k in INPUTS[:1] + INPUTS[2:] + ("features", "workspace"):
        _refused(fn, _plan(hxs_out=getattr(_plan(), k)), "hxs_out overlaps", k)
    _refused(fn, _plan(hxs_out=_plan().x + 4 * 10 * 64 * 4 - 8), "hxs_out overlaps x")             # the last bytes of x
    _refused(fn, _plan(hxs_out=_plan().hxs + 256), "hxs_out overlaps hxs")                          # a shifted overlap with hxs
    _refused(fn, _plan(hxs_out=_plan().hxs), "forward-only")                                        # a training plan: backward reads hxs
    if not torch.cuda.is_available():
        lib = _lib.load()
        p = _plan(hxs_out=_plan().hxs, workspace=None, workspace_bytes=0)
        assert lib.gmpe_gru_forward(0, C.byref(p), None) == -2, lib.gmpe_last_error().decode()      # accepted by the host checks


def _layer(D=64, H=64, **over):
    z = torch.zeros
    rnn = types.SimpleNamespace(weight_ih_l0=z(3 * H, D), weight_hh_l0=z(3 * H, H), bias_ih_l0=z(3 * H), bias_hh_l0=z(3 * H))
    norm = types.SimpleNamespace(weight=torch.ones(H), bias=z(H), eps=1e-5)
    layer = types.SimpleNamespace(rnn=rnn, norm=norm, _recurrent_N=1)
    for k, v in over.items():
        owner, _, name = k.rpartition("__")
        obj = getattr(layer, owner) if owner else layer
        if v is None:
            delattr(obj, name)
        else:
            setattr(obj, name, v)
    return layer


def test_python_layer_refuses_what_it_does_not_support():
    z = torch.zeros
    assert gmpe.rnn_layer is gmpe.gru.rnn_layer and gmpe.rnn_workspace_bytes is gmpe.gru.rnn_workspace_bytes
    x, hxs, m = z(20, 64), z(5, 1, 64), torch.ones(20, 1)
    with pytest.raises(NotImplementedError, match="recurrent_N = 2"):
        gmpe.rnn_layer(x, hxs, m, _layer(_recurrent_N=2))
    with pytest.raises(NotImplementedError, match="recurrent_N == 1"):
        gmpe.rnn_layer(x, z(5, 2, 64), m, _layer())
    with pytest.raises(NotImplementedError, match="more than one layer"):
        gmpe.rnn_layer(x, hxs, m, _layer(rnn__weight_ih_l1=z(192, 64)))
    with pytest.raises(NotImplementedError, match=r"\(in_dim, hidden\) = \(32, 64\)"):
        gmpe.rnn_layer(z(20, 32), hxs, m, _layer(D=32))
    with pytest.raises(NotImplementedError, match=r"\(in_dim, hidden\) = \(64, 128\)"):
        gmpe.rnn_layer(x, z(5, 1, 128), m, _layer(H=128))
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(NotImplementedError, match="float32 only"):
            gmpe.rnn_layer(x.to(dt), hxs, m, _layer())
        with pytest.raises(NotImplementedError, match="weight_hh is"):
            gmpe.rnn_layer(x, hxs, m, _layer(rnn__weight_hh_l0=z(192, 64, dtype=dt)))
    with pytest.raises(ValueError, match="x must be float32"):
        gmpe.rnn_layer(x.double(), hxs, m, _layer())
    with pytest.raises(ValueError, match="masks must be float32"):
        gmpe.rnn_layer(x, hxs, m.bool(), _layer())
    with pytest.raises(ValueError, match="hxs must be a tensor"):
        gmpe.rnn_layer(x, None, m, _layer())
    with pytest.raises(ValueError, match="no multiple of the 5 rows"):
        gmpe.rnn_layer(z(21, 64), hxs, torch.ones(21, 1), _layer())
    with pytest.raises(ValueError, match=r"masks must have shape \(20, 1\)"):
        gmpe.rnn_layer(x, hxs, torch.ones(19, 1), _layer())
    with pytest.raises(ValueError, match="x must have shape"):
        gmpe.rnn_layer(z(4, 5, 64), hxs, m, _layer())
    with pytest.raises(ValueError, match=r"weight_ih must have shape \(192, 64\)"):
        gmpe.rnn_layer(x, hxs, m, _layer(rnn__weight_ih_l0=z(128, 64)))
    with pytest.raises(ValueError, match=r"layer\.rnn\.bias_hh_l0 is missing"):
        gmpe.rnn_layer(x, hxs, m, _layer(rnn__bias_hh_l0=None))
    with pytest.raises(ValueError, match=r"layer\.norm\.weight is missing"):
        gmpe.rnn_layer(x, hxs, m, _layer(norm__weight=None))
    with pytest.raises(ValueError, match="layer must have .rnn"):
        gmpe.rnn_layer(x, hxs, m, types.SimpleNamespace(norm=None))
    with pytest.raises(ValueError, match="no CPU fallback"):                # everything else in order: the arrays are not on a device
        gmpe.rnn_layer(x, hxs, m, _layer())
    with pytest.raises(ValueError, match="no CPU fallback"):                # the reference's own layer object is accepted as it is
        gmpe.rnn_layer(x, hxs, m, types.SimpleNamespace(rnn=torch.nn.GRU(64, 64), norm=torch.nn.LayerNorm(64), _recurrent_N=1))


# ---------------------------------------------------------------------------------------------- (c)
def test_no_kernel_of_the_file_uses_scratch_memory():
    names, scratch = list(abi_lib.kernels("gru")), list(abi_lib.scratch("gru", "k_gru").values())
    assert len(names) == len(scratch) == 5 and all(s == 0 for s in scratch), (names, scratch)       # forward (two plans), bptt, wgrad, finish
    for k in ("k_gru_fwd", "k_gru_bptt", "k_gru_wgrad", "k_gru_finish"):
        assert any(k in n for n in names), k
