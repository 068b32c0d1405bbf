"""Host side of the policy's MLPBase (include/gmpe.h gmpe_mlp_forward / gmpe_mlp_backward, gmpe.mlp_base), no GPU:
(a) the float64 restatement of tests/mlp_lib.py agrees with the reference's own float32 run (tests/golden/mlp_base.npz, made by
    tests/golden/make_mlp_fixture.py) under the project's parity bar, 1e-5, per array; its backward is the derivative of its forward; every ReLU case
    meets the margin condition;
(b) the exported symbols, the plan's layout against the C header, and the refusals of both layers, which need no device;
(c) the compiler's resource report of csrc/gmpe_mlp.hip shows no scratch memory."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import abi_lib
import gmpe
import mlp_lib as M
from gmpe import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "mlp_base.npz"))


# ---------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("case", M.CASES, ids=M.key)
def test_the_restatement_agrees_with_the_reference_run_under_the_cap(case):
    _, _, t = M.truth64(case)
    assert list(t) == M.out_names(case)
    for k, v in t.items():
        ref = GOLD["%s_%s" % (M.key(case), k)]
        assert ref.dtype == np.float32 and ref.shape == v.shape, k
        e = M.err(ref, v)
        print("%s %-16s err_ref %.3g" % (M.key(case), k, e))
        assert e < M.CAP, (case, k, e)


@pytest.mark.parametrize("case", M.CASES, ids=M.key)
def test_the_relu_margin_holds_and_the_inputs_hold_what_they_promise(case):
    rows, dims, _, act, _ = case
    seed = M.seed_of(case)
    x = M.inputs(case, seed)["x"]
    assert x.shape == (rows, sum(dims)) and [p.shape[1] for p in M.split(x, dims)] == list(dims)
    if rows > 2:
        assert (x[1] == x[1, 0]).all() and x[1, 0] != 0 and (x[2] == 0).all()          # zero variance twice, once at zero mean
    if act == "ReLU":
        m = M.margin(case, seed)
        print("%s seed %d margin %.3g" % (M.key(case), seed, m))
        assert m >= M.MARGIN and all(M.margin(case, s) < M.MARGIN for s in range(seed))        # the first seed that meets it


def test_the_cases_are_the_listed_ones():
    assert M.TILE == _lib.MLP_ROW_TILE and len(M.CASES) == 12 and len(set(M.CASES)) == 12
    assert (65, (256,), 2, "ReLU", 1) in M.CASES and (33, (13, 16, 1, 1), 1, "ReLU", 1) in M.CASES and (2, (2,), 1, "ReLU", 1) in M.CASES
    assert sorted(GOLD.files) == sorted("%s_%s" % (M.key(c), k) for c in M.CASES for k in M.out_names(c))


@pytest.mark.parametrize("case", [(4, (3, 2), 2, "Tanh", 1), (4, (5,), 1, "ReLU", 1), (3, (2, 2), 0, "Tanh", 0)], ids=M.key)
def test_backward64_is_the_derivative_of_forward64(case):
    """the hand-written float64 backward against central differences of the float64 forward, on a few coordinates of every input"""
    seed = M.seed_of(case)
    P, I = M.params(case, seed), M.inputs(case, seed)
    g = M.backward64(I["x"], P, I["gf"], case)
    x64, P64 = I["x"].astype(np.float64), {k: v.astype(np.float64) for k, v in P.items()}
    loss = lambda: float((M.forward64(x64, P64, case) * I["gf"]).sum())
    rng = np.random.RandomState(0)
    for name in ["grad_x"] + ["grad_" + k for k in M.param_names(case)]:
        arr = x64 if name == "grad_x" else P64[name[5:]]
        for _ in range(4):
            i = tuple(rng.randint(0, s) for s in arr.shape)
            if name == "grad_x" and i[0] in (1, 2):
                continue                                # the zero-variance rows: rstd = 1 / sqrt(eps), a step of 1e-6 is not small there
            old, hstep = arr[i], 1e-6
            arr[i] = old + hstep
            up = loss()
            arr[i] = old - hstep
            dn = loss()
            arr[i] = old
            num = (up - dn) / (2 * hstep)
            assert abs(num - g[name][i]) <= 2e-6 * max(1.0, abs(num)), (name, i, num, g[name][i])


# ---------------------------------------------------------------------------------------------- (b)
def test_symbols_are_exported_and_the_plan_matches_the_header():
    lib = _lib.load()
    assert {"gmpe_mlp_workspace_bytes", "gmpe_mlp_forward", "gmpe_mlp_backward"} <= set(_lib.SYMBOLS) & abi_lib.exported()
    assert lib.gmpe_abi_version() == 3 and gmpe.config.ABI_VERSION == 3 == abi_lib.constant("GMPE_ABI_VERSION")   # added entry points: the ABI version stays
    for T in (_lib.GmpeMlpLayer, _lib.GmpeMlpPlan):
        assert abi_lib.layout(T) == abi_lib.mirror_layout(T), T
    names = ("ROW_TILE", "MAX_PARTS", "MAX_IN", "MAX_LAYERS", "RELU", "TANH")
    assert [abi_lib.constant("GMPE_MLP_" + k) for k in names] == [getattr(_lib, "MLP_" + k) for k in names]
    assert C.sizeof(_lib.GmpeMlpLayer) == 9 * 8 and C.sizeof(_lib.GmpeMlpPlan) == 8 + 6 * 4 + 4 * 8 + 4 * 4 + 4 * 8 + 5 * 8 + 3 * 72 + 4 * 8


def test_workspace_bytes():
    lib = _lib.load()
    n = C.c_size_t(7)
    assert lib.gmpe_mlp_workspace_bytes(1000, 29, 64, 1, 0, C.byref(n)) == 0 and n.value == 0          # the forward-only plan takes none
    sizes = []
    for rows in (1, 31, 32, 33, 1000, 40960, 512000):
        assert lib.gmpe_mlp_workspace_bytes(rows, 29, 64, 1, 1, C.byref(n)) == 0
        # the pre-activation gradients of both layers, the first layer's output, the feature norm's statistics
        assert n.value >= rows * (2 * 64 + 64 + 2) * 4 and n.value % 8 == 0
        sizes.append(n.value)
        assert gmpe.mlp_workspace_bytes(rows, 29, 1) == n.value and gmpe.mlp_workspace_bytes(rows, 29, 1, backward=False) == 0
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)                 # monotone in rows
    for layer_n in (0, 1, 2):                                                       # and in what a row keeps
        assert lib.gmpe_mlp_workspace_bytes(1000, 256, 64, layer_n, 1, C.byref(n)) == 0
        assert n.value >= 1000 * ((2 * layer_n + 1) * 64 + 2) * 4
    for args, field in (((0, 29, 64, 1, 1), "rows"), ((-5, 29, 64, 1, 1), "rows"), ((5, 0, 64, 1, 1), "in_dim"), ((5, 257, 64, 1, 1), "in_dim"),
                        ((5, 29, 32, 1, 1), "hidden"), ((5, 29, 64, 3, 1), "layer_n"), ((5, 29, 64, -1, 1), "layer_n"), ((5, 29, 64, 1, 2), "want_backward")):
        assert lib.gmpe_mlp_workspace_bytes(*args, C.byref(n)) == -1
        msg = lib.gmpe_last_error().decode()
        assert msg.startswith("gmpe_mlp_workspace_bytes:") and field in msg, msg
    assert lib.gmpe_mlp_workspace_bytes(5, 29, 64, 1, 1, None) == -1 and "bytes_out" in lib.gmpe_last_error().decode()
    with pytest.raises(NotImplementedError, match="hidden = 32"):
        gmpe.mlp_workspace_bytes(10, 29, 1, hidden=32)
    with pytest.raises(NotImplementedError, match="layer_N = 3"):
        gmpe.mlp_workspace_bytes(10, 29, 3)
    with pytest.raises(NotImplementedError, match="D_in = 300"):
        gmpe.mlp_workspace_bytes(10, 300, 1)


MB = 1 << 20
LAYER_IN = ("weight", "bias", "ln_weight", "ln_bias")


def _plan(**over):
    """a plan over fake, well separated addresses (1 MiB apart): nothing here reaches a device. over: field=value, `layer1__weight`, `part__1`"""
    p = _lib.GmpeMlpPlan()
    dims, layers = (13, 16), 2
    p.rows, p.hidden, p.layer_n, p.activation, p.feature_norm, p.n_parts, p.fn_eps = 70, 64, layers - 1, _lib.MLP_RELU, 1, len(dims), 1e-5
    addr = iter(range(MB, 200 * MB, MB))
    for i, d in enumerate(dims):
        p.part[i], p.part_dim[i], p.grad_part[i] = next(addr), d, next(addr)
    for k in ("fn_weight", "fn_bias", "grad_fn_weight", "grad_fn_bias", "features", "grad_features", "workspace"):
        setattr(p, k, next(addr))
    for l in range(layers):
        p.layer[l].eps = 1e-5
        for k in LAYER_IN + tuple("grad_" + k for k in LAYER_IN):
            setattr(p.layer[l], k, next(addr))
    p.workspace_bytes = MB
    for k, v in over.items():
        owner, _, name = k.rpartition("__")
        if owner.startswith("layer"):
            setattr(p.layer[int(owner[5:])], name, v)
        elif owner:
            getattr(p, owner)[int(name)] = v
        else:
            setattr(p, k, v)
    return p


def _refused(fn, plan, *names):
    lib = _lib.load()
    assert getattr(lib, fn)(0, C.byref(plan), None) == -1
    msg = lib.gmpe_last_error().decode()
    assert msg.startswith(fn + ":") and all(n in msg for n in names), msg
    return msg


@pytest.mark.parametrize("fn", ["gmpe_mlp_forward", "gmpe_mlp_backward"])
def test_c_entry_points_refuse_bad_plans_before_any_device_call(fn):
    lib = _lib.load()
    bwd = fn == "gmpe_mlp_backward"
    assert getattr(lib, fn)(0, None, None) == -1 and "null plan" in lib.gmpe_last_error().decode()
    for bad, name in ((dict(rows=0), "rows"), (dict(rows=-2), "rows"), (dict(rows=1 << 41), "rows"), (dict(hidden=128), "hidden"), (dict(hidden=0), "hidden"),
                      (dict(layer_n=3), "layer_n"), (dict(layer_n=-1), "layer_n"), (dict(activation=2), "activation"), (dict(feature_norm=2), "feature_norm"),
                      (dict(n_parts=0), "n_parts"), (dict(n_parts=5), "n_parts"), (dict(part_dim__0=0), "part_dim[0]"), (dict(part_dim__1=-4), "part_dim[1]"),
                      (dict(part_dim__1=257), "part_dim[1]"), (dict(part_dim__0=250), "sum of part_dim"), (dict(fn_eps=0.0), "fn_eps"),
                      (dict(fn_eps=float("nan")), "fn_eps"), (dict(layer0__eps=0.0), "layer[0].eps"), (dict(layer1__eps=-1.0), "layer[1].eps"),
                      (dict(workspace_bytes=64), "workspace_bytes"), (dict(workspace=5 * MB + 4), "workspace"), (dict(part__0=MB + 2), "part[0]"),
                      (dict(layer1__bias=MB + 1), "layer[1].bias"), (dict(features=MB + 2), "features")):
        _refused(fn, _plan(**bad), name)
    needed = ["part__0", "part__1", "fn_weight", "fn_bias"] + ["layer%d__%s" % (l, k) for l in (0, 1) for k in LAYER_IN]
    needed += ["grad_part__0", "grad_part__1", "grad_fn_weight", "grad_fn_bias", "grad_features", "workspace"] + \
        ["layer%d__grad_%s" % (l, k) for l in (0, 1) for k in LAYER_IN] if bwd else ["features"]
    for k in needed:
        owner, _, name = k.rpartition("__")
        label = "layer[%s].%s" % (owner[5:], name) if owner.startswith("layer") else "%s[%s]" % (owner, name) if owner else k
        _refused(fn, _plan(**{k: None}), label, "required")
    # layer 2 of a layer_n == 1 plan is not read, the feature norm's fields are not without feature_norm
    p = _plan(feature_norm=0, fn_weight=None, fn_bias=None, grad_fn_weight=None, grad_fn_bias=None, fn_eps=0.0, features=None, grad_features=None)
    _refused(fn, p, "grad_features" if bwd else "features")                         # ... so the first complaint is about the last thing checked


def test_what_each_entry_point_does_not_need_may_be_null():
    """a forward-only plan: no gradient pointers, no workspace; a backward plan: no features. The plans pass the host's checks and fail at the first device
    call (there is no device here): the error is not an argument error."""
    lib = _lib.load()
    grads = ["grad_part__0", "grad_part__1", "grad_fn_weight", "grad_fn_bias", "grad_features"] + ["layer%d__grad_%s" % (l, k) for l in (0, 1) for k in LAYER_IN]
    for fn, nulls in (("gmpe_mlp_forward", grads + ["workspace"]), ("gmpe_mlp_backward", ["features"])):
        p = _plan(**{k: None for k in nulls})
        if "workspace" in nulls:
            p.workspace_bytes = 0
        if torch.cuda.is_available():
            continue                                    # fake addresses must not reach a real device
        assert getattr(lib, fn)(0, C.byref(p), None) == -2, lib.gmpe_last_error().decode()          # GMPE_ERR_HIP: every host check passed


def _seq(K, act="ReLU", H=64, eps=1e-5, dtype=torch.float32):
    z = torch.zeros
    lin = types.SimpleNamespace(weight=z(H, K, dtype=dtype), bias=z(H, dtype=dtype))
    norm = types.SimpleNamespace(weight=torch.ones(H, dtype=dtype), bias=z(H, dtype=dtype), eps=eps)
    return [lin, type(act, (), {})(), norm]


def _base(D=29, layer_n=1, act="ReLU", fnorm=True, H=64, **over):
    mlp = types.SimpleNamespace(fc1=_seq(D, act, H), fc2=[_seq(H, act, H) for _ in range(layer_n)], _layer_N=layer_n)
    base = types.SimpleNamespace(mlp=mlp, _use_feature_normalization=fnorm,
                                 feature_norm=types.SimpleNamespace(weight=torch.ones(D), bias=torch.zeros(D), eps=1e-5))
    for k, v in over.items():
        owner, _, name = k.rpartition("__")
        obj = eval("base." + owner) if owner else base
        if v is None:
            delattr(obj, name)
        else:
            setattr(obj, name, v)
    return base


def test_python_layer_refuses_what_it_does_not_support():
    z = torch.zeros
    assert gmpe.mlp_base is gmpe.mlp.mlp_base and gmpe.mlp_workspace_bytes is gmpe.mlp.mlp_workspace_bytes
    obs, nbd = z(20, 13), z(20, 16)
    # NotImplementedError: what is not built
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(NotImplementedError, match=r"parts\[1\] is .*float32 only"):
            gmpe.mlp_base((obs, nbd.to(dt)), _base())
        with pytest.raises(NotImplementedError, match=r"fc1.weight is"):
            gmpe.mlp_base((obs, nbd), _base(mlp__fc1=_seq(29, dtype=dt)))
    with pytest.raises(NotImplementedError, match="hidden = 128"):
        gmpe.mlp_base((obs, nbd), _base(H=128))
    with pytest.raises(NotImplementedError, match="layer_N = 3"):
        gmpe.mlp_base((obs, nbd), _base(layer_n=3))
    with pytest.raises(NotImplementedError, match="D_in = 257"):
        gmpe.mlp_base((z(20, 256), z(20, 1)), _base(D=257))
    with pytest.raises(NotImplementedError, match="5 parts"):
        gmpe.mlp_base((obs, nbd, obs, nbd, obs), _base(D=71))
    with pytest.raises(NotImplementedError, match="activation GELU"):
        gmpe.mlp_base((obs, nbd), _base(act="GELU"))
    # ValueError: what is malformed
    with pytest.raises(ValueError, match=r"parts\[1\] must be a tensor"):
        gmpe.mlp_base((obs, None), _base())
    with pytest.raises(ValueError, match="parts must be a tensor or a tuple"):
        gmpe.mlp_base(None, _base())
    with pytest.raises(ValueError, match="at least one"):
        gmpe.mlp_base((), _base())
    with pytest.raises(ValueError, match=r"parts\[0\] must be float32"):
        gmpe.mlp_base((obs.double(), nbd), _base())
    with pytest.raises(ValueError, match=r"parts\[1\] has 19 rows, parts\[0\] has 20"):
        gmpe.mlp_base((obs, z(19, 16)), _base())
    with pytest.raises(ValueError, match=r"parts\[0\] must have shape \(rows, d\)"):
        gmpe.mlp_base((z(4, 5, 13), nbd), _base())
    with pytest.raises(ValueError, match=r"parts\[1\] must have shape \(rows, d\)"):
        gmpe.mlp_base((obs, z(20, 0)), _base())
    with pytest.raises(ValueError, match=r"fc1.weight must have shape \(64, 30\)"):
        gmpe.mlp_base((obs, z(20, 17)), _base(fnorm=False))
    with pytest.raises(ValueError, match=r"feature_norm.weight must have shape \(29,\)"):
        gmpe.mlp_base((obs, nbd), _base(feature_norm__weight=torch.ones(28)))
    short = _base()
    short.mlp._layer_N = 2
    with pytest.raises(ValueError, match="fc2 holds 1 layers, fewer than layer_N = 2"):
        gmpe.mlp_base((obs, nbd), short)
    with pytest.raises(ValueError, match=r"base\.mlp\.fc1\[0\]\.bias is missing"):
        gmpe.mlp_base((obs, nbd), _base(mlp__fc1=[types.SimpleNamespace(weight=z(64, 29))] + _seq(29)[1:]))
    with pytest.raises(ValueError, match=r"base\.feature_norm\.bias is missing"):
        gmpe.mlp_base((obs, nbd), _base(feature_norm__bias=None))
    with pytest.raises(ValueError, match="base must have .mlp"):
        gmpe.mlp_base((obs, nbd), types.SimpleNamespace())
    with pytest.raises(ValueError, match=r"must hold \[0\] the Linear"):
        gmpe.mlp_base((obs, nbd), _base(mlp__fc1=_seq(29)[:2]))
    # everything else in order: the arrays are not on a device. A single tensor stands for a 1-tuple; without feature normalisation no feature_norm is read
    with pytest.raises(ValueError, match="no CPU fallback"):
        gmpe.mlp_base((obs, nbd), _base())
    with pytest.raises(ValueError, match="no CPU fallback"):
        gmpe.mlp_base(z(20, 29), _base(fnorm=False, feature_norm=None))
    with pytest.raises(ValueError, match="no CPU fallback"):
        gmpe.mlp_base([obs, nbd, z(20, 1), z(20, 1)], _base(D=31, layer_n=2, act="Tanh"))
    # a torch module stack of the reference's shape is accepted as it is
    fc = lambda K: torch.nn.Sequential(torch.nn.Linear(K, 64), torch.nn.Tanh(), torch.nn.LayerNorm(64))
    mod = types.SimpleNamespace(_use_feature_normalization=True, feature_norm=torch.nn.LayerNorm(29),
                                mlp=types.SimpleNamespace(fc1=fc(29), fc2=torch.nn.ModuleList([fc(64)]), _layer_N=1))
    with pytest.raises(ValueError, match="no CPU fallback"):
        gmpe.mlp_base((obs, nbd), mod)


# ---------------------------------------------------------------------------------------------- (c)
def test_no_kernel_of_the_file_uses_scratch_memory():
    assert "mlp" in abi_lib.ru_objects()                                                            # `make resource-usage` holds it
    names, scratch = list(abi_lib.kernels("mlp")), list(abi_lib.scratch("mlp", "k_mlp").values())
    assert len(names) == len(scratch) == 4 and all(s == 0 for s in scratch), (names, scratch)       # forward, bprop, wgrad, finish
    for k in ("k_mlp_fwd", "k_mlp_bprop", "k_mlp_wgrad", "k_mlp_finish"):
        assert any(k in n for n in names), k
