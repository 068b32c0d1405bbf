"""Host side of the critic's value head and of the rollout half of gmpe.policy (include/gmpe.h gmpe_value_forward / gmpe_value_backward,
gmpe.value_head, gmpe.policy.get_actions / get_values / collect_step / compute / rollout / iteration), no GPU:
(a) tests/value_lib.py's float32 emulation of the forward's fixed order against a float64 dot product, within 64 * 2^-24 * sum|f * w| per row: 4 + 4 + 1
    roundings of at most 2^-24 relative each lie on a row's path, each on a partial sum that sum|f * w| bounds (times 1 + a few 2^-24), so 64 is generous;
    and its float64 emulation of the backward's fixed order against float32(math.fsum(exact products)) on signed g, up to 34 tiles, with inputs on which
    each level of that order shows;
(b) the exported symbols, the plan against the C header, the workspace size against the restated geometry, the C entries' refusals;
(c) every refusal and argument error of value_head and of the new policy functions, raised on CPU tensors before any device call;
(d) the compiler's resource report of csrc/gmpe_value.hip shows no scratch memory."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import abi_lib
import gmpe
import value_lib as VL
from gmpe import _lib, policy
from gmpe.rollout import DeviceRolloutBuffer

MB = 1 << 20


# ---------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("source", ["random", "shipped"])
@pytest.mark.parametrize("rows", VL.ROWS)
def test_the_emulation_is_a_dot_product(rows, source):
    f, w, b, _ = VL.inputs(rows, source)
    got = VL.emulate(f, w, b)
    want = np.asarray(f, np.float64) @ np.asarray(w, np.float64).reshape(-1) + float(b[0])
    bound = 64 * 2.0 ** -24 * VL.sum_abs(f, w)
    worst = float((np.abs(got.astype(np.float64) - want) / bound).max())
    print("rows %d %s: worst |emulation - float64| / bound %.3g" % (rows, source, worst))
    assert got.dtype == np.float32 and got.shape == (rows,) and worst <= 1.0
    assert np.abs(want).max() > 0.01
    # a row's bits are the row's alone
    assert np.array_equal(VL.bits(VL.emulate(f[rows // 2:rows // 2 + 1], w, b)), VL.bits(got[rows // 2:rows // 2 + 1]))


def test_the_emulation_keeps_the_stated_order():
    """inputs on which the order shows: with a lane's four products 2^24, 1, 1, -2^24 the lane's sum from 0.0f ascending is 0 (the ones are absorbed),
    where a float64 sum rounded once gives 2; the xor tree adds lane pairs (0, 1), (2, 3) first"""
    f, w = np.zeros((1, 64), np.float32), np.ones((1, 64), np.float32)
    f[0, :4] = [2.0 ** 24, 1.0, 1.0, -2.0 ** 24]
    assert VL.emulate(f, w, np.zeros(1, np.float32))[0] == 0.0
    f[:] = 0.0
    f[0, [0, 4, 8, 12]] = [2.0 ** 24, 1.0, 1.0, -2.0 ** 24]      # lanes 0 .. 3: (2^24 + 1) + (1 - 2^24) = 2^24 + (1 - 2^24) = 1: one 1 is absorbed
    assert VL.emulate(f, w, np.zeros(1, np.float32))[0] == 1.0                     # an ascending chain gives 0, the once-rounded sum 2
    f[:] = 0.0
    f[0, [0, 8, 12, 4]] = [2.0 ** 24, 1.0, 1.0, -2.0 ** 24]      # lanes 0, 1 hold +-2^24: they cancel first, the ones survive
    assert VL.emulate(f, w, np.zeros(1, np.float32))[0] == 2.0


@pytest.mark.parametrize("rows", VL.ROWS + VL.MANY_ROWS)
def test_the_backward_emulation_is_the_once_rounded_sum(rows):
    """signed g, so the sums cancel: the emulation's order of double adds must still land on float32(the exact sum) or its float32 neighbour in every
    column and in the bias. With these seeds it is exact in all 64 columns and in the bias at every row count, the smallest |sum| / sum|terms| of a
    column being 1.7e-4 (256 rows): the neighbour is slack the reference does not use."""
    f, _, _, g = VL.inputs(rows)
    assert (g < 0).any() and (g > 0).any() or rows == 1
    gw, gb = VL.emulate_backward(f, g)
    assert gw.dtype == gb.dtype == np.float32 and gw.shape == (1, 64) and gb.shape == (1,)
    products = g.astype(np.float64) * f.astype(np.float64)                  # exact: float32 x float32 fits a double
    want_w, want_b = VL.once_rounded(products), VL.once_rounded(g.astype(np.float64))
    ratio = np.abs(products.sum(0)) / np.abs(products).sum(0)
    print("rows %d: the emulation is exact in %d of 64 columns, min |sum| / sum|terms| %.3g; bias exact: %s"
          % (rows, int((gw.reshape(-1) == want_w).sum()), float(ratio.min()), bool(gb[0] == want_b[0])))
    assert (VL.neighbours(want_w) == gw.reshape(1, 64)).any(0).all(), (gw, want_w)
    assert (VL.neighbours(want_b) == gb.reshape(1, 1)).any(), (gb, want_b)
    if rows in VL.MANY_ROWS:                                                # the inputs can see a finish that loses tile 16
        lost_w, lost_b = VL.emulate_backward(f, g, skip_tiles=(16,))
        assert not np.array_equal(VL.bits(lost_w), VL.bits(gw)) and VL.bits(lost_b)[0] != VL.bits(gb)[0]


def _spike(rows, at):
    """grad_weight[0, 0] and grad_bias of `rows` rows with g = 1 and column 0 holding 2^60, 1, 1, -2^60 in the rows `at`, zeros elsewhere: 2 where the
    order lets the two 2^60 cancel first, 0 where a 1 is added to 2^60 (whose double ulp is 256) and lost"""
    f = np.zeros((rows, 64), np.float32)
    f[list(at), 0] = [2.0 ** 60, 1.0, 1.0, -2.0 ** 60]
    gw, gb = VL.emulate_backward(f, np.ones((rows, 1), np.float32))
    assert gb[0] == rows and not gw[0, 1:].any()
    return float(gw[0, 0])


def test_the_backward_emulation_keeps_the_stated_order():
    assert _spike(13, (0, 4, 8, 12)) == 0.0             # one lane's passes 0 .. 3, ascending: ((2^60 + 1) + 1) - 2^60
    assert _spike(13, (0, 8, 12, 4)) == 2.0             # ... 2^60 - 2^60 in passes 0 and 1, then the ones
    assert _spike(4, (0, 2, 3, 1)) == 2.0               # the four row groups of pass 0: (2^60 - 2^60) + (1 + 1)
    assert _spike(4, (0, 1, 3, 2)) == 0.0               # ... (2^60 + 1) + (-2^60 + 1)
    assert _spike(4, (0, 1, 2, 3)) == 0.0               # ... (2^60 + 1) + (1 - 2^60)
    assert _spike(193, (0, 64, 128, 192)) == 0.0        # the four waves in wave order
    assert _spike(193, (0, 128, 192, 64)) == 2.0        # ... waves 0 and 1 hold the two 2^60: ((2^60 - 2^60) + 1) + 1
    assert _spike(4097, (0, 256, 512, 4096)) == 2.0     # tiles 0 and 16 share slice 0 and cancel there; an ascending sum over the tiles would give 0
    assert _spike(4097, (0, 4096, 512, 256)) == 1.0     # ... slice 0 = 2^60 + 1 loses tile 16's 1, then slice 1 = -2^60 and slice 2 = 1; ascending tiles: 2
    one = np.random.RandomState(3).randn(1, 64).astype(np.float32)
    gw, gb = VL.emulate_backward(one, np.float32([[-1.5]]))
    assert np.array_equal(VL.bits(gw), VL.bits(np.float32(-1.5) * one)) and gb[0] == -1.5       # one row: one exact product, rounded once


# ---------------------------------------------------------------------------------------------- (b)
def test_symbols_are_exported_and_the_plan_matches_the_header():
    lib = _lib.load()
    assert {"gmpe_value_workspace_bytes", "gmpe_value_forward", "gmpe_value_backward"} <= set(_lib.SYMBOLS) & abi_lib.exported()
    assert lib.gmpe_abi_version() == 3 and gmpe.config.ABI_VERSION == 3          # added entry points: the ABI version stays
    assert abi_lib.layout(_lib.GmpeValuePlan) == abi_lib.mirror_layout(_lib.GmpeValuePlan) and C.sizeof(_lib.GmpeValuePlan) == 8 + 2 * 4 + 10 * 8
    assert ("int", "gmpe_value_forward", ["int", "const gmpe_value_plan*", "void*"]) in abi_lib.prototypes()
    assert ("int", "gmpe_value_workspace_bytes", ["int64_t", "int32_t", "size_t*"]) in abi_lib.prototypes()
    assert gmpe.value_head is gmpe.value.value_head and gmpe.value_workspace_bytes is gmpe.value.value_workspace_bytes and gmpe.value.HIDDEN == 64
    for name in ("get_actions", "get_values", "collect_step", "compute", "rollout", "iteration"):
        assert callable(getattr(gmpe.policy, name))


def test_workspace_bytes_and_the_restated_geometry():
    lib = _lib.load()
    n = C.c_size_t(7)
    assert lib.gmpe_value_workspace_bytes(100, 0, C.byref(n)) == 0 and n.value == 0                     # the forward-only plan takes none
    for rows, want in ((1, 640), (256, 640), (257, 1280), (1025, 5 * 640), (40960, 160 * 640), (512000, 2000 * 640)):
        assert lib.gmpe_value_workspace_bytes(rows, 1, C.byref(n)) == 0
        assert n.value == want == VL.workspace_bytes(rows) == gmpe.value_workspace_bytes(rows) and gmpe.value_workspace_bytes(rows, backward=False) == 0
    for args, field in (((0, 1), "rows"), ((-3, 1), "rows"), (((1 << 40) + 1, 1), "rows"), ((10, 2), "want_backward")):
        assert lib.gmpe_value_workspace_bytes(*args, C.byref(n)) == -1
        msg = lib.gmpe_last_error().decode()
        assert msg.startswith("gmpe_value_workspace_bytes:") and field in msg, msg
    assert lib.gmpe_value_workspace_bytes(10, 1, None) == -1 and "bytes_out" in lib.gmpe_last_error().decode()


PTRS = ("features", "weight", "bias", "values_out", "grad_values", "grad_features", "grad_weight", "grad_bias", "workspace")


def _plan(**over):
    """a value plan over fake, well separated addresses: nothing here reaches a device"""
    p = _lib.GmpeValuePlan()
    p.rows, p.hidden, p.workspace_bytes = 70, 64, 64 * MB
    for i, k in enumerate(PTRS):
        setattr(p, k, (i + 1) * MB)
    for k, v in over.items():
        setattr(p, k, v)
    return p


def _refused(fn, args, *names):
    lib = _lib.load()
    assert getattr(lib, fn)(0, *args, None) == -1
    msg = lib.gmpe_last_error().decode()
    assert msg.startswith(fn + ":") and all(n in msg for n in names), msg


@pytest.mark.parametrize("fn", ["gmpe_value_forward", "gmpe_value_backward"])
def test_c_entry_points_refuse_bad_plans_before_any_device_call(fn):
    bwd = fn == "gmpe_value_backward"
    _refused(fn, (None,), "null plan")
    for bad, name in ((dict(rows=0), "rows"), (dict(rows=(1 << 40) + 1), "rows"), (dict(hidden=32), "hidden"), (dict(hidden=128), "hidden"),
                      (dict(features=MB + 2), "features"), (dict(weight=MB + 1), "weight"), (dict(bias=MB + 3), "bias"),
                      (dict(values_out=MB + 2), "values_out"), (dict(grad_values=MB + 2), "grad_values"), (dict(grad_features=MB + 1), "grad_features"),
                      (dict(grad_weight=MB + 2), "grad_weight"), (dict(grad_bias=MB + 2), "grad_bias"), (dict(workspace=5 * MB + 4), "workspace")):
        _refused(fn, (C.byref(_plan(**bad)),), name)
    for k in (("features", "weight", "grad_values", "workspace") if bwd else ("features", "weight", "bias", "values_out")):
        _refused(fn, (C.byref(_plan(**{k: None})),), k, "required")
    if bwd:
        _refused(fn, (C.byref(_plan(workspace_bytes=VL.workspace_bytes(70) - 8)),), "workspace_bytes", str(VL.workspace_bytes(70)))


def test_what_each_entry_point_does_not_need_may_be_null():
    """the plans pass the host's checks and fail at the first device call (there is no device here): the error is not an argument error"""
    lib = _lib.load()
    if torch.cuda.is_available():
        return                                          # fake addresses must not reach a real device
    grads = {k: None for k in ("grad_values", "grad_features", "grad_weight", "grad_bias", "workspace")}
    assert lib.gmpe_value_forward(0, C.byref(_plan(workspace_bytes=0, **grads)), None) == -2, lib.gmpe_last_error().decode()
    assert lib.gmpe_value_backward(0, C.byref(_plan(bias=None, values_out=None, grad_features=None, grad_bias=None)), None) == -2


# ---------------------------------------------------------------------------------------------- (c)
class _PopArt(object):
    def __init__(self):
        self.weight, self.bias = torch.nn.Parameter(torch.zeros(1, 64)), torch.nn.Parameter(torch.zeros(1))


def test_value_head_refuses_what_it_does_not_support():
    z = torch.zeros
    f, lin = z(10, 64), torch.nn.Linear(64, 1)
    # NotImplementedError: what is not built
    with pytest.raises(NotImplementedError, match="H = 32"):
        gmpe.value_head(z(10, 32), torch.nn.Linear(32, 1))
    with pytest.raises(NotImplementedError, match="hidden = 64"):
        gmpe.value_head(z(10, 32), lin)
    with pytest.raises(NotImplementedError, match="2 output rows"):
        gmpe.value_head(f, torch.nn.Linear(64, 2))
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(NotImplementedError, match="critic_features is .*float32 only"):
            gmpe.value_head(f.to(dt), lin)
        with pytest.raises(NotImplementedError, match=r"v_out.weight is .*float32 only"):
            gmpe.value_head(f, torch.nn.Linear(64, 1).to(dt))
    # ValueError: what is malformed or misplaced
    with pytest.raises(ValueError, match="critic_features must be a tensor"):
        gmpe.value_head(None, lin)
    with pytest.raises(ValueError, match="critic_features must be float32"):
        gmpe.value_head(f.double(), lin)
    with pytest.raises(ValueError, match="critic_features must have shape"):
        gmpe.value_head(z(10, 2, 64), lin)
    with pytest.raises(ValueError, match="critic_features must be contiguous"):
        gmpe.value_head(z(64, 10).t(), lin)
    with pytest.raises(ValueError, match="v_out.bias is missing"):
        gmpe.value_head(f, torch.nn.Linear(64, 1, bias=False))
    with pytest.raises(ValueError, match="v_out.weight is missing"):
        gmpe.value_head(f, types.SimpleNamespace())
    with pytest.raises(ValueError, match="shapes"):
        gmpe.value_head(f, types.SimpleNamespace(weight=z(64), bias=z(1)))
    with pytest.raises(ValueError, match="only without gradients"):
        gmpe.value_head(f, lin, out=z(10))
    with torch.no_grad():
        with pytest.raises(ValueError, match="out must be a contiguous float32 tensor with 10 elements"):
            gmpe.value_head(f, lin, out=z(11))
        with pytest.raises(ValueError, match="out must be a contiguous float32 tensor"):
            gmpe.value_head(f, lin, out=z(10, dtype=torch.float64))
        # everything else in order: the arrays are not on a device (an nn.Linear, a PopArt)
        for v_out in (lin, _PopArt()):
            with pytest.raises(ValueError, match="no CPU fallback"):
                gmpe.value_head(f, v_out, out=z(10, 1))
    with pytest.raises(ValueError, match="no CPU fallback"):
        gmpe.value_head(f, lin)


def _fake_buffer(**over):
    """what the rollout entries read of a DeviceRolloutBuffer before they touch the device, on the CPU"""
    N, A, T = 2, 3, 4
    b = types.SimpleNamespace(engine=types.SimpleNamespace(N=N, A=A), step=0, T=T, value_preds=torch.zeros(T + 1, N, A, 1), returns=torch.zeros(T + 1, N, A, 1),
                              _node_obs=torch.zeros(T + 1, N, A, 5, 7), _adj=torch.zeros(T + 1, N, 5, 5), rnn_states=torch.zeros(T + 1, N, A, 1, 64),
                              rnn_states_critic=torch.zeros(T + 1, N, A, 1, 64), act_outputs=None, act_finish=None,
                              args=types.SimpleNamespace(use_popart=False, use_valuenorm=True))
    b._flags = types.MethodType(DeviceRolloutBuffer._flags, b)
    for k, v in over.items():
        setattr(b, k, v)
    return b


def test_the_rollout_entries_refuse_before_any_device_call():
    rnn_net, bare_net = types.SimpleNamespace(rnn=object()), types.SimpleNamespace()
    calls = {"collect_step": lambda b, a=rnn_net, c=rnn_net: policy.collect_step(a, c, b), "rollout": lambda b, a=rnn_net, c=rnn_net: policy.rollout(a, c, b),
             "compute": lambda b, a=None, c=rnn_net: policy.compute(c, b)}
    for fn, call in calls.items():
        with pytest.raises(ValueError, match="buffer must be a DeviceRolloutBuffer: %s reads buffer" % fn):
            call(types.SimpleNamespace(step=0))
        with pytest.raises(ValueError, match="%s needs a buffer with value_preds" % fn):
            call(_fake_buffer(value_preds=None))
        with pytest.raises(ValueError, match="%s reads node_obs rows" % fn):
            call(_fake_buffer(_node_obs=None))
        with pytest.raises(ValueError, match="%s reads an adjacency" % fn):
            call(_fake_buffer(_adj=None))
        with pytest.raises(ValueError, match="the critic has an RNN: %s needs a buffer with rnn_states_critic" % fn):
            call(_fake_buffer(rnn_states_critic=None))
    for fn in ("collect_step", "rollout"):
        with pytest.raises(ValueError, match="the actor has an RNN: %s needs a buffer with rnn_states" % fn):
            calls[fn](_fake_buffer(rnn_states=None))
        with pytest.raises(ValueError, match="the critic has an RNN"):
            calls[fn](_fake_buffer(rnn_states=None, rnn_states_critic=None), a=bare_net)    # an actor without an RNN needs none; the critic's are missed
    for fn in ("rollout", "compute"):
        with pytest.raises(ValueError, match="%s needs a buffer with value_preds and returns" % fn):
            calls[fn](_fake_buffer(returns=None))
    with pytest.raises(ValueError, match="rollout starts at buffer.step == 0, not 2"):
        policy.rollout(rnn_net, rnn_net, _fake_buffer(step=2))
    with pytest.raises(ValueError, match="compute needs the runner's args"):
        policy.compute(bare_net, _fake_buffer(args=None))
    with pytest.raises(ValueError, match="compute: args.use_valuenorm / use_popart is set, so a value_normalizer is required"):
        policy.compute(bare_net, _fake_buffer())
    with pytest.raises(ValueError, match="out must be a dict"):
        policy.get_actions(bare_net, bare_net, *([None] * 9), seed=0, num_agents=1, draw=0, out=[torch.zeros(3)])


def test_the_learner_entries_refuse_an_unknown_value_head_before_anything_else():
    for fn, call in (("minibatch_losses", lambda **k: policy.minibatch_losses(None, None, None, None, **k)),
                     ("ppo_update", lambda **k: policy.ppo_update(None, None, None, None, None, None, **k)),
                     ("train", lambda **k: policy.train(None, None, None, None, None, None, **k)),
                     ("iteration", lambda **k: policy.iteration(None, None, None, None, None, None, **k))):
        with pytest.raises(ValueError, match='value_head = \'hip\': %s takes "torch"' % fn):
            call(value_head="hip")
    with pytest.raises(TypeError):
        policy.minibatch_losses(None, None, (1,) * 16, None, None, "replace", None, None, "device")        # keyword-only
    with pytest.raises(NotImplementedError, match="accumulation_steps = 2: iteration"):
        policy.iteration(None, None, None, None, None, None, accumulation_steps=2)
    with pytest.raises(NotImplementedError, match="shards: iteration"):
        policy.iteration(None, None, None, None, None, None, shards=object())
    with pytest.raises(ValueError, match="16-tuple"):
        policy.minibatch_losses(None, None, (1, 2, 3), None, value_head="device")


# ---------------------------------------------------------------------------------------------- (d)
def test_no_kernel_of_the_file_uses_scratch_memory():
    assert "value" in abi_lib.ru_objects()                                                          # `make resource-usage` holds it
    names, scratch = list(abi_lib.kernels("value")), list(abi_lib.scratch("value", "k_value").values())
    assert len(names) == len(scratch) == 5 and all(s == 0 for s in scratch), (names, scratch)       # forward and backward's rows in both load widths, the finish
    for k in ("k_value_fwd", "k_value_bwd_rows", "k_value_finish"):
        assert any(k in n for n in names), k
