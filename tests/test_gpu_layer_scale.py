"""The GRU and MLPBase kernels at the sizes where a workgroup owns several tiles (tests/layer_scale_lib.py names the paths and the shapes that reach them;
tests/test_layer_scale_host.py proves the reach without a device):
(a) accuracy under the project's rule, err_dev <= 4 * err_ref + 2^-23 per array with err_ref from the CPU float32 reference;
(b) a row on a later tile has the bits of the same row in a call of its own;
(c) every row reaches every sum exactly once, with no tolerance: integer column sums, and loss weights that are zero but in one row;
(d) the C entries at scale: the wrapper's bits, guard rows behind every output, guard bytes behind the workspace, a second backward with the same bits."""
import functools

import numpy as np
import pytest
import torch

import gmpe
import gru_lib as G
import layer_scale_lib as S
import mlp_lib as M
import test_gpu_gru as TG
import test_gpu_mlp as TM

pytestmark = pytest.mark.gpu
DEV = TM.DEV
MLP_LOOP = [c for c in S.MLP_CASES if "loop_bwd" in S.MLP_REACH[c]]             # 8257 and 32801 rows
MLP_BIG, MLP_RELU, GRU_BIG = S.MLP_CASES[2], S.MLP_CASES[3], S.GRU_CASES[2]
MLP_ROWWISE = lambda case: ["features"] + ["grad_part%d" % i for i in range(len(case[1]))]
GRU_ROWWISE = ("features", "hxs_out", "grad_x", "grad_hxs")
WORST = {}


def worst(kernel, got, ref32, t64, names, lib):
    w = max(lib.err(got[k], t64[k]) / lib.bound(lib.err(ref32[k], t64[k])) for k in names)
    WORST[kernel] = max(WORST.get(kernel, 0.0), w)
    print("%s: worst err_dev / bound %.3f here, %.3f so far" % (kernel, w, WORST[kernel]))


@functools.lru_cache(maxsize=None)
def mlp_full(case):
    I, P, _ = S.mlp_truth(case)
    return TM.run(case, I["x"], I["gf"], P)


@functools.lru_cache(maxsize=None)
def gru_full(L, Nb, pattern):
    I, m, P, _ = S.gru_truth(L, Nb, pattern)
    return TG.run(I, m, P)


def poisoned(nbytes):
    """a workspace whose old contents are NaNs in every format: what a kernel fails to write shows"""
    return torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)


def mlp_params_of(case):
    return ["grad_" + k for k in M.param_names(case)]


def gru_rows(I, m, idx, L, Nb):
    """the inputs and masks of rows idx of every step, as a batch of len(idx) rows"""
    sel = lambda a: np.ascontiguousarray(a.reshape(L, Nb, a.shape[-1])[:, idx]).reshape(-1, a.shape[-1])
    return dict(x=sel(I["x"]), hxs=np.ascontiguousarray(I["hxs"][idx]), gf=sel(I["gf"]), gh=np.ascontiguousarray(I["gh"][idx])), sel(m)


def gru_cut(out, k, idx, L, Nb):
    a = out[k]
    return a.reshape(L, Nb, a.shape[-1])[:, idx] if k in ("features", "grad_x") else a.reshape(1, Nb, G.H)[:, idx]


# ---------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("case", S.MLP_CASES, ids=M.key)
def test_mlp_accuracy_at_scale(case):
    _, _, t64 = S.mlp_truth(case)
    got, ref32 = mlp_full(case), S.mlp_reference(case)
    worst("mlp", got, ref32, t64, M.out_names(case), M)
    TM.check(got, ref32, t64, M.key(case), M.out_names(case))


@pytest.mark.parametrize("L,Nb", S.GRU_CASES)
@pytest.mark.parametrize("pattern", S.GRU_PATTERNS)
def test_gru_accuracy_at_scale(L, Nb, pattern):
    _, _, _, t64 = S.gru_truth(L, Nb, pattern)
    got, ref32 = gru_full(L, Nb, pattern), S.gru_reference(L, Nb, pattern)
    worst("gru", got, ref32, t64, TG.OUT, G)
    TG.check(got, ref32, t64, G.key(L, Nb, pattern))


# ---------------------------------------------------------------------------------------------- (b)
def mlp_slices(case):
    first = S.mlp_geometry_of(case)["grid_fwd"] * S.MLP_TILE        # everything a second iteration of the tile loop produced, and tile 0 with a row of tile 1
    assert first in (256 * 32, 1024 * 32) and first < case[0]
    return [(first, case[0]), (0, 33)]


@pytest.mark.parametrize("case", MLP_LOOP, ids=M.key)
def test_mlp_rows_of_a_later_tile_have_the_bits_of_a_call_of_their_own(case):
    I, P, _ = S.mlp_truth(case)
    full = mlp_full(case)
    for a, b in mlp_slices(case):
        got = TM.run((b - a,) + case[1:], I["x"][a:b], I["gf"][a:b], P)
        for k in MLP_ROWWISE(case):
            assert TM.same(got[k], full[k][a:b]), "rows %d .. %d: %s" % (a, b - 1, k)


def test_mlp_forward_only_plan_on_later_tiles():
    case = MLP_RELU
    I, P, _ = S.mlp_truth(case)
    base, _ = TM.make_base(P, case)
    training = mlp_full(case)["features"]
    fwd = lambda a, b: gmpe.mlp_base(tuple(TM.dev(q) for q in M.split(I["x"][a:b], case[1])), base).cpu().numpy()
    with torch.no_grad():
        f = fwd(0, case[0])
        assert TM.same(f, training)                     # the training plan runs the same forward
        for a, b in mlp_slices(case):
            assert TM.same(fwd(a, b), f[a:b]), "rows %d .. %d" % (a, b - 1)


def test_gru_rows_of_a_later_tile_have_the_bits_of_a_call_of_their_own():
    L, Nb = GRU_BIG
    I, m, P, _ = S.gru_truth(L, Nb, "random")
    full = gru_full(L, Nb, "random")
    first = S.gru_geometry(L, Nb)["grid"] * S.GRU_TILE
    late = np.arange(first, Nb)
    assert first == 8192 and len(late) == 65
    J, mj = gru_rows(I, m, late, L, Nb)
    got = TG.run(J, mj, P)
    for k in GRU_ROWWISE:
        assert TG.same(gru_cut(got, k, np.arange(len(late)), L, len(late)), gru_cut(full, k, late, L, Nb)), "rows 8192 .. 8256 alone: " + k
    perm = np.concatenate([late, np.arange(first)])     # the same rows in tiles 0 .. 2, the others behind them
    J, mj = gru_rows(I, m, perm, L, Nb)
    got = TG.run(J, mj, P)
    for k in GRU_ROWWISE:
        assert TG.same(gru_cut(got, k, np.arange(Nb), L, Nb), gru_cut(full, k, perm, L, Nb)), "permuted batch: " + k


# ---------------------------------------------------------------------------------------------- (c)
@pytest.mark.parametrize("shift", S.INTEGER_SHIFTS)
@pytest.mark.parametrize("case", [S.MLP_CASES[0]] + MLP_LOOP, ids=M.key)
def test_mlp_integer_column_sums_are_exact(case, shift):
    """the gradient of the last LayerNorm's bias is the column sum of the loss weights: small integers, exact in any order, so one dropped or doubled row
    in the lanes' sums, the wave add or the slices shows"""
    I, P, _ = S.mlp_truth(case)
    gf = S.integer_gf(case[0], shift)
    got = TM.run(case, I["x"], gf, P, workspace=poisoned(S.mlp_geometry_of(case)["workspace"]))["grad_lnb%d" % case[2]]
    want = gf.astype(np.int64).sum(0)
    assert np.array_equal(got.astype(np.float64), want.astype(np.float64)), (got - want).tolist()


@pytest.mark.parametrize("shift", S.INTEGER_SHIFTS)
@pytest.mark.parametrize("L,Nb", [S.GRU_CASES[0], GRU_BIG])
def test_gru_integer_column_sums_are_exact(L, Nb, shift):
    I, m, P, _ = S.gru_truth(L, Nb, "random")
    gf = S.integer_gf(L * Nb, shift)
    got = TG.run(I, m, P, gf=gf, gh=np.zeros_like(I["gh"]), workspace=poisoned(S.gru_geometry(L, Nb)["workspace"]))["grad_ln_bias"]
    want = gf.astype(np.int64).sum(0)
    assert np.array_equal(got.astype(np.float64), want.astype(np.float64)), (got - want).tolist()


def mlp_one_hot_rows(case):
    g = S.mlp_geometry_of(case)
    rows = {"the last row": case[0] - 1, "row 32 of part 64": 64 * g["part_rows"] + S.PART_ROWS, "row 0": 0}
    if g["ntiles"] > g["grid_bwd"]:
        rows["the first row of the second pass"] = g["grid_bwd"] * S.MLP_TILE
    assert g["part_rows"] > S.PART_ROWS and all(0 <= r < case[0] for r in rows.values())
    return rows


@pytest.mark.parametrize("case", [S.MLP_CASES[1], MLP_BIG], ids=M.key)
def test_mlp_one_row_reaches_every_parameter_gradient_once(case):
    """loss weights that are zero but in row r: every other row contributes exact zeros and a product of two float32 values is exact in double, so every
    parameter gradient of the full call has the value of the one-row call on row r (+0 and -0 compare equal)"""
    I, P, _ = S.mlp_truth(case)
    ws = poisoned(S.mlp_geometry_of(case)["workspace"])
    for what, r in mlp_one_hot_rows(case).items():
        gf = S.one_hot_gf(case[0], r, seed=r)
        full = TM.run(case, I["x"], gf, P, workspace=ws)
        one = TM.run((1,) + case[1:], I["x"][r:r + 1], gf[r:r + 1], P)
        for k in mlp_params_of(case):
            assert np.abs(one[k]).max() > 0, k
            assert np.array_equal(full[k], one[k]), "%s (%d): %s differs by up to %.3g" % (what, r, k, np.abs(full[k] - one[k]).max())
        for k in MLP_ROWWISE(case)[1:]:
            assert TM.same(full[k][r:r + 1], one[k]) and not np.delete(full[k], r, 0).any(), (what, k)


def test_gru_one_row_reaches_every_parameter_gradient_once():
    """as above for rows 8256 and 8192 of (2, 8257), with loss weights on both steps of the row and on its final state: two terms per sum, in different
    parts, so their grouping cannot matter"""
    L, Nb = GRU_BIG
    I, m, P, _ = S.gru_truth(L, Nb, "ones")
    ws = poisoned(S.gru_geometry(L, Nb)["workspace"])
    for r in (Nb - 1, S.gru_geometry(L, Nb)["grid"] * S.GRU_TILE):
        gf, gh = np.zeros((L, Nb, G.H), np.float32), np.zeros_like(I["gh"])
        rng = np.random.RandomState(6100 + r)
        gf[:, r], gh[r] = rng.randn(L, G.H), rng.randn(1, G.H)
        K = dict(I, gf=gf.reshape(L * Nb, G.H), gh=gh)
        full = TG.run(K, m, P, workspace=ws)
        J, mj = gru_rows(K, m, np.array([r]), L, Nb)
        one = TG.run(J, mj, P)
        for k in ["grad_" + n for n in G.PARAMS]:
            assert np.abs(one[k]).max() > 0, k
            assert np.array_equal(full[k], one[k]), "row %d: %s differs by up to %.3g" % (r, k, np.abs(full[k] - one[k]).max())


def test_gru_the_last_row_of_a_ragged_part_before_empty_parts():
    """(17, 241): time-major row m = 4096 is the last row of part 124, parts 125 .. 127 hold no row. With the mask of (t = 16, row 240) zero the gradient
    stops at that step, so it is the only row with a nonzero gate gradient, and every parameter gradient is that of the (1, 1) call on it."""
    L, Nb = S.GRU_CASES[1]
    I, m, P, _ = S.gru_truth(L, Nb, "ones")
    mm = L * Nb - 1
    assert mm == 4096 and [q for q, (m0, m1) in enumerate(S.part_ranges(L * Nb)) if m0 <= mm < m1] == [124]
    m = m.copy()
    m[mm] = 0
    gf = S.one_hot_gf(L * Nb, mm, seed=1)
    K = dict(I, gf=gf, gh=np.zeros_like(I["gh"]))
    full = TG.run(K, m, P, workspace=poisoned(S.gru_geometry(L, Nb)["workspace"]))
    J = dict(x=I["x"][mm:mm + 1], hxs=I["hxs"][Nb - 1:Nb], gf=gf[mm:mm + 1], gh=np.zeros((1, 1, G.H), np.float32))
    one = TG.run(J, np.zeros((1, 1), np.float32), P)
    for k in ["grad_" + n for n in G.PARAMS]:
        assert np.abs(one[k]).max() > 0 or k == "grad_weight_hh", k               # the masked previous state is zero
        assert np.array_equal(full[k], one[k]), "%s differs by up to %.3g" % (k, np.abs(full[k] - one[k]).max())
    assert TG.same(full["grad_x"][mm:mm + 1], one["grad_x"]) and not full["grad_x"][:mm].any() and not full["grad_hxs"].any()


# ---------------------------------------------------------------------------------------------- (d)
@pytest.mark.parametrize("fill", [0, 0xFF])
def test_the_mlp_c_entries_at_scale(fill):
    I, P, _ = S.mlp_truth(MLP_BIG)
    a, b = mlp_full(MLP_BIG), TM.c_call(MLP_BIG, I, P, fill=fill)            # c_call: guard rows, guard bytes behind the workspace, two backward calls
    for k in M.out_names(MLP_BIG):
        assert TM.same(a[k], b[k]), k


@pytest.mark.parametrize("fill", [0, 0xFF])
def test_the_gru_c_entries_at_scale(fill):
    L, Nb = GRU_BIG
    I, m, P, _ = S.gru_truth(L, Nb, "random")
    a, b = gru_full(L, Nb, "random"), TG.c_call(I, m, P, fill=fill)
    for k in TG.OUT:
        assert TG.same(a[k], b[k]), k
