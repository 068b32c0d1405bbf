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
half an ulp. Two calls with the same rows give the same bits."""
import types

import numpy as np
import pytest
import torch

import gmpe
import value_lib as VL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = 5


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
    """the `values` gmpe_ppo_loss_popart evaluates for these features, weight and bias"""
    rows = f.shape[0]
    rng = np.random.RandomState(5 + rows)
    col = lambda a: _dev(a.astype(np.float32).reshape(rows, 1))
    fields = dict(actions=col(rng.randint(0, K, rows)), value_preds=col(rng.randn(rows)), returns=col(rng.randn(rows)), active_masks=col(np.ones(rows)),
                  old_action_log_probs=col(-rng.rand(rows)), adv_targ=col(rng.randn(rows)))
    args = types.SimpleNamespace(use_popart=True, use_valuenorm=False)
    res = gmpe.ppo_losses_popart(_dev(rng.randn(rows, K).astype(np.float32)), _dev(f), fields, args, _PopArt(w, b))
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
