"""gmpe.value_head — the critic's v_out on the device (csrc/gmpe_value.hip) — at rows 1, 63, 64, 65, 255, 256, 257 and 1025: the edges of a wave, of a 256-row
tile, and one row past four tiles.
Forward: the bits are tests/value_lib.py's emulation of the stated order, and those of the `values` ppo_losses_popart evaluates for the same features,
weight and bias; a row's bits do not depend on the batch it is evaluated in; out= is written in place.
Backward through autograd: grad_features is the float32 product g * W bit for bit; grad_weight and grad_bias are float32(math.fsum(exact products)) or its
float32 neighbour — the device adds at most 1025 exact double products in double (each add within 2^-53 relative of its partial sum) and rounds once, so
it can miss the once-rounded exact sum by more than one float32 ulp only where the partial sums dwarf the result, i.e. where the terms cancel. grad_bias
is a plain sum of g, so the case that pins it takes g in (0.5, 1.5): every partial sum is below the total and the double sum's error is below
1025 * 2^-53 of it, far under half a float32 ulp; for grad_weight (g * F with F ~ N(0, 1) changes sign) the same case is held to the neighbours too,
with |sum| / sum|terms| of every column printed and asserted above 2^-20: an error of 1025 * 2^-53 * sum|terms| is then below 2^-22.9 |sum|, under
half an ulp. Two calls with the same rows give the same bits.
With signed g, where the sums cancel, and up to 8449 rows (34 tiles, so that the finish's 16 slices hold up to three tiles each) grad_weight and grad_bias
are held bit for bit to value_lib.emulate_backward, the float64 restatement of the device's order: every step is an IEEE double add of exact products.
The C entries are driven directly with caller-owned buffers (c_call): NaN guards around every output, a workspace of exactly the queried size with old
contents, each pointer aligned or 4 bytes off on its own, every subset of the three gradients, a second backward on one plan, a side stream, a captured
graph; and the values a rollout stores are compared with those ppo_losses_popart evaluates on minibatches of other sizes."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

import gmpe
import value_lib as VL
from gmpe import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = 5
GUARD = 64                                              # bytes behind the workspace and behind every output, which the kernels must leave alone
NAN = float("nan")
GRADS = ("grad_features", "grad_weight", "grad_bias")


class _PopArt(object):
    """the tensors of a PopArt(64, 1) around a given weight and bias, fresh statistics"""

    def __init__(self, w, b):
        t = lambda a: torch.from_numpy(np.array(a, np.float32)).to(DEV)
        self.beta, self.epsilon, self.norm_axes, self.output_shape = 0.99999, 1e-5, 1, 1
        self.weight, self.bias = torch.nn.Parameter(t(w)), torch.nn.Parameter(t(b))
        self.stddev, self.mean, self.mean_sq = t(np.ones(1)), t(np.zeros(1)), t(np.zeros(1))
        self.debiasing_term = torch.zeros((), device=DEV)


def _linear(w, b, grad=True):
    lin = torch.nn.Linear(64, 1).to(DEV)
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(np.array(w)))
        lin.bias.copy_(torch.from_numpy(np.array(b)))
    return lin.requires_grad_(grad)


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _popart_values(f, w, b):
    """the `values` gmpe_ppo_loss_popart evaluates for these features (an array, or a device tensor taken where it lies), weight and bias"""
    rows = int(f.shape[0])
    rng = np.random.RandomState(5 + rows)
    col = lambda a: _dev(a.astype(np.float32).reshape(rows, 1))
    fields = dict(actions=col(rng.randint(0, K, rows)), value_preds=col(rng.randn(rows)), returns=col(rng.randn(rows)), active_masks=col(np.ones(rows)),
                  old_action_log_probs=col(-rng.rand(rows)), adv_targ=col(rng.randn(rows)))
    args = types.SimpleNamespace(use_popart=True, use_valuenorm=False)
    res = gmpe.ppo_losses_popart(_dev(rng.randn(rows, K).astype(np.float32)), f if isinstance(f, torch.Tensor) else _dev(f), fields, args, _PopArt(w, b))
    return res.values


@pytest.mark.parametrize("source", ["random", "shipped"])
@pytest.mark.parametrize("rows", VL.ROWS)
def test_forward_bits(rows, source):
    f, w, b, _ = VL.inputs(rows, source)
    want = VL.bits(VL.emulate(f, w, b))
    fd, lin = _dev(f), _linear(w, b, grad=False)
    values = gmpe.value_head(fd, lin)
    assert tuple(values.shape) == (rows, 1) and values.dtype == torch.float32 and not values.requires_grad
    pop = _PopArt(w, b)
    with torch.no_grad():
        from_popart = gmpe.value_head(fd, pop)              # the duck-typed PopArt: the same two tensors
    in_loss = _popart_values(f, w, b)
    # out=: a slot of a larger array, written in place, the neighbours untouched
    slab = torch.full((3, rows, 1), 7.0, device=DEV)
    ret = gmpe.value_head(fd, lin, out=slab[1])
    assert ret.data_ptr() == slab[1].data_ptr() and tuple(ret.shape) == (rows, 1)
    # a view that starts 4 bytes into an allocation: the 4-byte loads give the same bits
    odd = torch.empty(rows * 64 + 1, device=DEV)[1:].view(rows, 64).copy_(fd)
    assert odd.data_ptr() % 16 == 4
    unaligned = gmpe.value_head(odd, lin)
    # chunks, and single rows
    cuts = sorted(set([0, 1, rows // 3, rows // 2, rows - 1, rows]))
    chunks = torch.cat([gmpe.value_head(fd[a:b_].contiguous(), lin) for a, b_ in zip(cuts[:-1], cuts[1:]) if b_ > a])
    alone = [(r, gmpe.value_head(fd[r:r + 1].contiguous(), lin)) for r in sorted(set([0, rows // 2, rows - 1]))]
    torch.cuda.synchronize()
    for name, got in (("value_head", values), ("PopArt v_out", from_popart), ("ppo_losses_popart.values", in_loss), ("out=", slab[1]), ("chunks", chunks),
                      ("4-byte loads", unaligned)):
        assert np.array_equal(VL.bits(got.cpu().numpy()), want), name
    for r, v in alone:
        assert VL.bits(v.cpu().numpy())[0] == want[r], r
    assert bool((slab[0] == 7.0).all()) and bool((slab[2] == 7.0).all())


@pytest.mark.parametrize("rows", VL.ROWS)
def test_backward_through_autograd(rows):
    f, w, b, g = VL.inputs(rows, "random", positive_g=True)
    assert (g > 0).all()                                    # no cancellation in grad_bias: see the head of this file
    runs = []
    for _ in range(2):
        fd, lin = _dev(f).requires_grad_(True), _linear(w, b)
        values = gmpe.value_head(fd, lin)
        assert values.requires_grad
        values.backward(_dev(g))
        runs.append((fd.grad, lin.weight.grad, lin.bias.grad))
    # features alone: the parameter sums are not formed, the products are the same
    fd, frozen = _dev(f).requires_grad_(True), _linear(w, b, grad=False)
    gmpe.value_head(fd, frozen).backward(_dev(g))
    # parameters alone, with the caller's workspace
    ws = torch.empty(gmpe.value_workspace_bytes(rows), dtype=torch.uint8, device=DEV)
    lin2 = _linear(w, b)
    gmpe.value_head(_dev(f), lin2, workspace=ws).backward(_dev(g))
    torch.cuda.synchronize()
    gf, gw, gb = (t.cpu().numpy() for t in runs[0])
    assert gf.shape == (rows, 64) and gw.shape == (1, 64) and gb.shape == (1,)
    assert np.array_equal(VL.bits(gf), VL.bits(g * w)), "grad_features is the float32 product"
    assert np.array_equal(VL.bits(fd.grad.cpu().numpy()), VL.bits(gf)) and frozen.weight.grad is None
    for a, b_ in zip(runs[0], runs[1]):
        assert np.array_equal(VL.bits(a.cpu().numpy()), VL.bits(b_.cpu().numpy())), "two calls with the same rows"
    assert np.array_equal(VL.bits(lin2.weight.grad.cpu().numpy()), VL.bits(gw)) and np.array_equal(VL.bits(lin2.bias.grad.cpu().numpy()), VL.bits(gb))
    products = g.astype(np.float64) * f.astype(np.float64)                  # exact: float32 x float32 fits a double
    want_w, want_b = VL.once_rounded(products), VL.once_rounded(g.astype(np.float64))
    ratio = np.abs(products.sum(0)) / np.abs(products).sum(0)
    off_w = np.flatnonzero(~(VL.neighbours(want_w) == gw.reshape(1, 64)).any(0))
    print("rows %d: grad_weight exact in %d of 64 columns, min |sum| / sum|terms| %.3g; grad_bias exact: %s"
          % (rows, int((gw.reshape(-1) == want_w).sum()), float(ratio.min()), bool(gb[0] == want_b[0])))
    assert (VL.neighbours(want_b) == gb.reshape(1, 1)).any(), (gb, want_b)
    assert float(ratio.min()) > 2.0 ** -20, "the seeded case cancels in a column: choose another seed"
    assert off_w.size == 0, (off_w, ratio[off_w], gw.reshape(-1)[off_w], want_w[off_w])


# ---------------------------------------------------------------------------------------------- many tiles, signed g
def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(VL.bits(a), VL.bits(b))


def wrapper_run(f, w, b, g):
    """gmpe.value_head + autograd with grad_values g -> values and the three gradients; f may be a device tensor, taken where it lies"""
    fd = (f.detach() if isinstance(f, torch.Tensor) else _dev(f)).requires_grad_(True)
    lin = _linear(w, b)
    values = gmpe.value_head(fd, lin)
    values.backward(_dev(g))
    torch.cuda.synchronize()
    return dict(values=values.detach().cpu().numpy(), grad_features=fd.grad.cpu().numpy(), grad_weight=lin.weight.grad.cpu().numpy(),
                grad_bias=lin.bias.grad.cpu().numpy())


@functools.lru_cache(maxsize=None)
def wrapped(rows):
    """the wrapper on VL.inputs(rows) (signed g), aligned: computed once, shared, never written to"""
    return wrapper_run(*VL.inputs(rows))


@pytest.mark.parametrize("rows", VL.ROWS + VL.MANY_ROWS)
def test_signed_g_gives_the_emulations_bits_up_to_34_tiles(rows):
    """4097 rows are 17 tiles (slice 0 of the finish holds two), 8449 rows 34 (slices 0 and 1 hold three, the others two; the last tile has one row)"""
    f, w, b, g = VL.inputs(rows)
    assert rows == 1 or ((g < 0).any() and (g > 0).any())
    got = wrapped(rows)
    want_w, want_b = VL.emulate_backward(f, g)
    assert got["values"].shape == (rows, 1) and np.array_equal(VL.bits(got["values"]), VL.bits(VL.emulate(f, w, b)))
    assert same(got["grad_features"], g * w), "grad_features is the float32 product"
    assert same(got["grad_weight"], want_w), np.flatnonzero(VL.bits(got["grad_weight"]) != VL.bits(want_w))
    assert same(got["grad_bias"], want_b), (got["grad_bias"], want_b)


@pytest.mark.parametrize("rows", VL.MANY_ROWS)
def test_the_last_row_alone_among_many_tiles_gives_the_one_row_calls_sums(rows):
    """with grad_values zero except in the last row every other row adds exact zeros to the double sums, in whatever tile and slice it lies"""
    f, w, b, g = VL.inputs(rows)
    g1 = np.zeros_like(g)
    g1[-1] = g[-1]
    many, one = wrapper_run(f, w, b, g1), wrapper_run(f[-1:], w, b, g[-1:])
    assert np.abs(one["grad_weight"]).max() > 0 and np.abs(one["grad_bias"]).max() > 0 and np.abs(one["grad_features"]).max() > 0
    assert same(many["grad_weight"], one["grad_weight"]) and same(many["grad_bias"], one["grad_bias"])
    assert same(many["grad_features"][-1:], one["grad_features"]) and not many["grad_features"][:-1].any()


# ---------------------------------------------------------------------------------------------- the C entries
def offset(a, off):
    """`a` on the device at `off` elements past an aligned base: off 0 takes the 16-byte path, 1 the 4-byte one"""
    a = np.array(a, np.float32)                         # a copy: the shared inputs are read-only
    buf = torch.empty(a.size + 8, dtype=torch.float32, device=DEV)
    v = buf[off:off + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == (off * 4) % 16
    return v


def guarded(n, off=0):
    """n floats with `off` floats in front of them and GUARD bytes behind, all NaN -> (the whole buffer, the view the kernel gets)"""
    buf = torch.full((n + GUARD // 4 + 8,), NAN, dtype=torch.float32, device=DEV)
    return buf, buf[off:off + n]


def untouched(buf, n, off=0):
    return bool(torch.isnan(buf[:off]).all()) and bool(torch.isnan(buf[off + n:]).all())


def c_call(rows, off=0, fill=0x00, stream=None, want=GRADS, arrays=None):
    """gmpe_value_forward, then gmpe_value_backward twice on one plan, through ctypes with caller-owned buffers `off` floats past an aligned base (one
    offset for every pointer, or a dict {plan field: offset} with the fields it does not name at 0). Backward writes the outputs named in `want` and gets
    neither bias nor values_out; its workspace has exactly the queried size, is pre-filled with `fill` and followed by GUARD bytes. Asserted here: nothing
    outside an output or behind the workspace is written, the second backward gives the first one's bits, and a call that asks for grad_features alone
    leaves the workspace as it was."""
    lib = _lib.load()
    f, w, b, g = arrays or VL.inputs(rows)
    o = (lambda k: off.get(k, 0)) if isinstance(off, dict) else (lambda k: off)
    fd, wd, bd, gd = offset(f, o("features")), offset(w, o("weight")), offset(b, o("bias")), offset(g, o("grad_values"))
    st = C.c_void_p((stream or torch.cuda.current_stream(torch.device(DEV))).cuda_stream)
    p = _lib.GmpeValuePlan()
    p.rows, p.hidden = rows, 64
    p.features, p.weight, p.bias = fd.data_ptr(), wd.data_ptr(), bd.data_ptr()
    vbuf, v = guarded(rows, off=o("values_out"))
    p.values_out = v.data_ptr()
    _lib.check(lib.gmpe_value_forward(0, C.byref(p), st), "gmpe_value_forward")
    torch.cuda.synchronize()
    assert untouched(vbuf, rows, o("values_out")), "values_out: written outside"
    res = {"values": v.cpu().numpy().reshape(rows, 1)}
    nbytes = gmpe.value_workspace_bytes(rows)
    assert nbytes == VL.workspace_bytes(rows)
    ws = torch.full((nbytes + GUARD,), fill, dtype=torch.uint8, device=DEV)
    shapes = dict(grad_features=(rows, 64), grad_weight=(1, 64), grad_bias=(1,))
    outs = {k: guarded(int(np.prod(shapes[k])), off=o(k)) for k in want}
    p.bias, p.values_out, p.grad_values = None, None, gd.data_ptr()                    # backward reads neither
    for k, (_, out) in outs.items():
        setattr(p, k, out.data_ptr())
    p.workspace, p.workspace_bytes = ws.data_ptr(), nbytes
    first = None
    for rep in range(2):                                # backward may be repeated on one plan: re-poisoned outputs, the same bits
        _lib.check(lib.gmpe_value_backward(0, C.byref(p), st), "gmpe_value_backward")
        torch.cuda.synchronize()
        if rep == 0:
            first = {k: out.clone() for k, (_, out) in outs.items()}
            for _, out in outs.values():
                out.fill_(NAN)
            torch.cuda.synchronize()
    assert bool((ws[nbytes:] == fill).all()), "bytes past the workspace were written"
    if "grad_weight" not in want and "grad_bias" not in want:
        assert bool((ws == fill).all()), "grad_features alone: the workspace was written"
    for k, (buf, out) in outs.items():
        assert untouched(buf, out.numel(), o(k)), k + ": written outside"
        assert same(out.cpu().numpy(), first[k].cpu().numpy()), "the second backward call differs: " + k
        res[k] = out.cpu().numpy().reshape(shapes[k])
    return res


C_ROWS = (1, 63, 257, 4097)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("rows", C_ROWS)
def test_the_c_entries_give_the_wrappers_bits_whatever_the_workspace_held_and_stay_inside_their_outputs(rows, off):
    """0xFF bytes are NaN doubles: a partial row that is read without having been written shows"""
    full = wrapped(rows)
    for fill in (0x00, 0xFF):
        got = c_call(rows, off=off, fill=fill)
        assert sorted(got) == sorted(full)
        for k in full:
            assert same(got[k], full[k]), (fill, k)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("rows", C_ROWS)
def test_a_side_stream_gives_the_same_bits(rows, off):
    full = wrapped(rows)
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        other = c_call(rows, off=off, fill=0xFF, stream=side)
        f, w, b, g = VL.inputs(rows)
        through = wrapper_run(offset(f, off), w, b, g)                              # the wrapper launches on the current stream
    for k in full:
        assert same(other[k], full[k]) and same(through[k], full[k]), k


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("rows", C_ROWS)
def test_every_subset_of_the_gradients_may_be_asked_for(rows, off):
    """the tiles' partial rows are written when grad_weight or grad_bias is wanted, either alone too: over a workspace of NaN doubles a finish that reads
    rows nobody wrote shows. Backward gets neither bias nor values_out in any of these calls."""
    full = wrapped(rows)
    for m in range(1, 8):
        want = tuple(k for i, k in enumerate(GRADS) if m >> i & 1)
        got = c_call(rows, off=off, fill=0xFF, want=want)
        assert sorted(got) == sorted(want + ("values",))
        for k in got:
            assert same(got[k], full[k]), (want, k)


@pytest.mark.parametrize("rows", [1, 65, 257, 4097])
def test_the_4_byte_backward_gives_the_aligned_calls_bits(rows):
    """backward moves features and grad_features in 4-byte units when either is not 16-byte aligned: through autograd from a features view 4 bytes into an
    allocation (autograd's own grad_features is aligned), through the C entry with grad_features alone 4 bytes off, and with both"""
    f, w, b, g = VL.inputs(rows)
    full = wrapped(rows)
    odd = offset(f, 1)
    assert odd.data_ptr() % 16 == 4 and odd.is_contiguous()
    runs = {"autograd, features off": wrapper_run(odd, w, b, g), "grad_features off": c_call(rows, off={"grad_features": 1}),
            "both off": c_call(rows, off={"features": 1, "grad_features": 1})}
    for name, got in runs.items():
        for k in full:
            assert same(got[k], full[k]), (name, k)


def test_a_captured_forward_and_backward_replay_on_new_inputs():
    """one forward and one backward captured on a single stream into static buffers; before each of three replays other features, grad_values, weight and
    bias are copied into the static inputs and the outputs and the workspace are poisoned"""
    lib = _lib.load()
    rows = 4097
    sets = []
    for i in range(3):
        rng = np.random.RandomState(70 + i)
        sets.append((rng.randn(rows, 64).astype(np.float32), (rng.randn(1, 64) / 8).astype(np.float32), (0.1 * rng.randn(1)).astype(np.float32),
                     rng.randn(rows, 1).astype(np.float32)))
    eager = [wrapper_run(*s) for s in sets]
    assert not same(eager[0]["grad_weight"], eager[1]["grad_weight"]) and not same(eager[1]["values"], eager[2]["values"])
    ins = [torch.zeros(s.shape, device=DEV) for s in sets[0]]
    shapes = dict(values=(rows, 1), grad_features=(rows, 64), grad_weight=(1, 64), grad_bias=(1,))
    outs = {k: torch.full(s, NAN, device=DEV) for k, s in shapes.items()}
    ws = torch.full((gmpe.value_workspace_bytes(rows),), 0xFF, dtype=torch.uint8, device=DEV)
    fwd, bwd = _lib.GmpeValuePlan(), _lib.GmpeValuePlan()
    for p in (fwd, bwd):
        p.rows, p.hidden, p.features, p.weight = rows, 64, ins[0].data_ptr(), ins[1].data_ptr()
    fwd.bias, fwd.values_out = ins[2].data_ptr(), outs["values"].data_ptr()
    bwd.grad_values, bwd.workspace, bwd.workspace_bytes = ins[3].data_ptr(), ws.data_ptr(), ws.numel()
    for k in GRADS:
        setattr(bwd, k, outs[k].data_ptr())

    def call():
        st = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
        _lib.check(lib.gmpe_value_forward(0, C.byref(fwd), st), "gmpe_value_forward")
        _lib.check(lib.gmpe_value_backward(0, C.byref(bwd), st), "gmpe_value_backward")
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                                      # eager, on a side stream as torch.cuda.graph wants for warm-up
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for i, s in enumerate(sets):
        for t, a in zip(ins, s):
            t.copy_(torch.from_numpy(a))
        for t in outs.values():
            t.fill_(NAN)
        ws.fill_(0xFF)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        for k, t in outs.items():
            assert same(t.cpu().numpy(), eager[i][k]), (i, k)


def test_a_rollouts_values_are_the_loss_values_on_minibatches_of_other_sizes():
    """value_preds as a rollout stores them — 4097 rows, out= into a slot of a buffer, no_grad — against ppo_losses_popart(...).values on two minibatches
    gathered from those rows, of other sizes and one of them 4 bytes off: the claim gmpe/value.py is written around. And the stride-0 grad_values that
    values.sum().backward() hands over give the bits of an explicit array of ones."""
    rows = 4097
    f, w, b, _ = VL.inputs(rows)
    fd, lin = _dev(f), _linear(w, b, grad=False)
    slab = torch.full((3, rows, 1), 7.0, device=DEV)
    with torch.no_grad():
        ret = gmpe.value_head(fd, lin, out=slab[1])
    assert ret.data_ptr() == slab[1].data_ptr()
    stored = slab[1].cpu().numpy()
    assert np.array_equal(VL.bits(stored), VL.bits(VL.emulate(f, w, b))) and bool((slab[0] == 7.0).all()) and bool((slab[2] == 7.0).all())
    perm = np.random.RandomState(11).permutation(rows - 1)
    for idx, off in ((np.concatenate([[rows - 1], perm[:299]]), 1), (perm[299:812], 0)):        # 300 rows with the last one among them, and 513
        mb = offset(f[idx], off)
        assert mb.data_ptr() % 16 == 4 * off and mb.shape[0] in (300, 513)
        in_loss = _popart_values(mb, w, b)
        torch.cuda.synchronize()
        assert same(in_loss.detach().cpu().numpy(), stored[idx]), (len(idx), off)
    fd2, lin2 = _dev(f).requires_grad_(True), _linear(w, b)
    gmpe.value_head(fd2, lin2).sum().backward()
    torch.cuda.synchronize()
    ones = wrapper_run(f, w, b, np.ones((rows, 1), np.float32))
    assert same(fd2.grad.cpu().numpy(), ones["grad_features"]) and same(fd2.grad.cpu().numpy(), np.broadcast_to(w, (rows, 64)))
    assert same(lin2.weight.grad.cpu().numpy(), ones["grad_weight"]) and same(lin2.bias.grad.cpu().numpy(), ones["grad_bias"])
    assert float(lin2.bias.grad[0]) == float(rows)
