"""What the tests of the GRU and MLPBase kernels at the sizes where a workgroup owns several tiles share (tests/test_layer_scale_host.py,
tests/test_gpu_layer_scale.py): a Python restatement of the launch geometry and the workspace layouts of csrc/gmpe_wgrad.h, csrc/gmpe_mlp.hip and
csrc/gmpe_gru.hip, the shapes with the path each was chosen for, and their inputs, float64 truths and CPU float32 references, computed once per process.

The paths (none is reached below 513 rows, all run at the training and rollout shapes):
  loop    the tile loop `for (tile = blockIdx.x; tile < ntiles; tile += gridDim.x)` runs twice in some workgroup: ntiles > grid;
  slices  sum_slices adds more than one partial row in some slice: n > FIN_SLICES (n: k_mlp_bprop's grid, the GRU's tiles);
  stages  part_products runs more than one LDS stage per part: part_rows > PART_ROWS; `ragged`: the last stage is not full;
  empty   MAX_PARTS parts of ceil(M / MAX_PARTS) rows overshoot M: trailing parts hold no row and still write zeros;
  straddle (GRU) a part holds rows on both sides of m = Nb, where the previous state switches from hxs to the saved h of step t - 1.

The ReLU rule at scale: over 2e6 pre-activations no seed keeps every one MARGIN away from zero, so the ReLU case draws mlp_lib's inputs and redraws, from
a seeded generator, exactly the rows whose smallest |pre-activation| in the float64 truth is below the margin, until none is left (rows 1 and 2, the
constant and the zero row, are never redrawn: if they miss the margin the next parameter seed is taken)."""
import functools

import numpy as np

import gru_lib as G
import mlp_lib as M

# csrc/gmpe_gru.hip, csrc/gmpe_mlp.hip, csrc/gmpe_wgrad.h, include/gmpe.h: tests/test_layer_scale_host.py reads them out of the sources
MAX_GRID = 256
MAX_CU, LDS_CU = 256, 160 * 1024
MAX_PARTS, PART_ROWS, FIN_SLICES = 128, 32, 16
MLP_TILE = GRU_TILE = 32
H = 64
MLP_NCOL, GRU_NCOL = 1088, 384                          # doubles per partial row of column sums

MLP_CASES = ((545, (13, 16), 1, "Tanh", 1), (4097, (67,), 0, "Tanh", 0), (8257, (256,), 2, "Tanh", 1), (32801, (13, 16), 1, "ReLU", 1))
GRU_CASES = ((8, 545), (17, 241), (2, 8257))
GRU_PATTERNS = ("random", "ones")
# the sizes the issue checked against a local build, next to the cases above
MLP_SIZE_SHAPES = ((1, 29, 1), (97, 67, 2), (4096, 29, 1), (512000, 29, 1)) + tuple((c[0], sum(c[1]), c[2]) for c in MLP_CASES)
GRU_SIZE_SHAPES = ((1, 1), (10, 65), (128, 32)) + GRU_CASES


def cdiv(a, b):
    return -(-a // b)


def partition(M_):
    """gmpe_wgrad::partition -> (nparts, part_rows)"""
    nparts = min(cdiv(M_, PART_ROWS), MAX_PARTS)
    return nparts, cdiv(M_, nparts)


def part_ranges(M_):
    """[m0, m1) of every part, m1 clamped to M as the wgrad kernels clamp it (m1 < m0 for a part past the end)"""
    nparts, pr = partition(M_)
    return [(q * pr, min(q * pr + pr, M_)) for q in range(nparts)]


def mlp_geometry(rows, D, layer_n):
    """layout() of csrc/gmpe_mlp.hip"""
    g = dict(ntiles=cdiv(rows, MLP_TILE), nblk1=cdiv(D, 64), DP=(D + 3) & ~3)
    g["DS"] = max(g["DP"], H)
    g["nparts"], g["part_rows"] = partition(rows)
    g["lds_fwd"] = (g["DP"] * (H + 1) + layer_n * H * (H + 1) + MLP_TILE * g["DS"]) * 4
    g["lds_bwd"] = max(g["lds_fwd"], 4 * MLP_NCOL * 8)
    g["grid_fwd"] = min(g["ntiles"], MAX_CU * min(4, max(1, LDS_CU // g["lds_fwd"])))
    g["grid_bwd"] = min(g["ntiles"], MAX_CU)
    n = g["grid_bwd"] * MLP_NCOL * 8 + g["nparts"] * (g["nblk1"] + layer_n) * H * H * 8 + rows * 16 + rows * (layer_n + 1) * 256 + rows * layer_n * 256
    g["workspace"] = (n + 7) & ~7
    return g


def gru_geometry(L, Nb):
    """layout() of csrc/gmpe_gru.hip"""
    g = dict(M=L * Nb, ntiles=cdiv(Nb, GRU_TILE))
    g["grid"] = min(g["ntiles"], MAX_GRID)
    g["nparts"], g["part_rows"] = partition(g["M"])
    n = g["ntiles"] * GRU_NCOL * 8 + g["nparts"] * 2 * 192 * H * 8 + g["M"] * (256 + 256 + 64 + 2) * 4
    g["workspace"] = (n + 7) & ~7
    return g


def mlp_geometry_of(case):
    return mlp_geometry(case[0], sum(case[1]), case[2])


def _parts_reach(M_):
    nparts, pr = partition(M_)
    return dict(stages=pr > PART_ROWS, ragged=pr > PART_ROWS and pr % PART_ROWS != 0, empty=any(m0 >= M_ for m0, _ in part_ranges(M_)))


def mlp_reach(case):
    g = mlp_geometry_of(case)
    r = dict(loop_fwd=g["ntiles"] > g["grid_fwd"], loop_bwd=g["ntiles"] > g["grid_bwd"], slices=g["grid_bwd"] > FIN_SLICES)
    r.update(_parts_reach(case[0]))
    return r


def gru_reach(L, Nb):
    g = gru_geometry(L, Nb)
    r = dict(loop=g["ntiles"] > g["grid"], slices=g["ntiles"] > FIN_SLICES, straddle=any(m0 < Nb < m1 for m0, m1 in part_ranges(g["M"])))
    r.update(_parts_reach(g["M"]))
    return r


# what each shape was chosen for: the host test asserts it, the GPU tests rely on it
MLP_REACH = {MLP_CASES[0]: ("slices",), MLP_CASES[1]: ("stages", "ragged", "empty"), MLP_CASES[2]: ("loop_fwd", "loop_bwd", "slices", "stages", "ragged"),
             MLP_CASES[3]: ("loop_fwd", "loop_bwd", "slices", "stages", "ragged")}
GRU_REACH = {GRU_CASES[0]: ("slices", "stages", "ragged", "straddle"), GRU_CASES[1]: ("stages", "ragged", "empty", "straddle"),
             GRU_CASES[2]: ("loop", "slices", "stages", "ragged", "straddle")}


INTEGER_SHIFTS = (-2, 1)


def integer_gf(rows, shift=-2):
    """loss weights (r * 7 + j) % 5 + shift: their column sums are exact in double and in float32 in any order. shift = -2 is signed and sums to zero over
    any 5 consecutive rows — so 65 dropped rows (8257 - 8192), or the 7680 rows of workgroups 16 .. 255, would not show; shift = 1 is positive, and every
    dropped or doubled set of rows changes every column's sum."""
    r, j = np.arange(rows, dtype=np.int64)[:, None], np.arange(H, dtype=np.int64)[None, :]
    return ((r * 7 + j) % 5 + shift).astype(np.float32)


def one_hot_gf(rows, r, seed=0):
    """loss weights that are zero but in row r (N(0, 1) there)"""
    gf = np.zeros((rows, H), np.float32)
    gf[r] = np.random.RandomState(6000 + seed).randn(H).astype(np.float32)
    return gf


# ---------------------------------------------------------------------------------------------- MLP
def _row_margin(x, P, case):
    _, s = M.forward64(x, P, case, keep=True)
    return np.min([np.abs(pre).min(1) for _, pre, _, _, _ in s["layers"]], axis=0)


@functools.lru_cache(maxsize=None)
def mlp_inputs(case):
    """-> (inputs, params, rows redrawn, parameter seed). A Tanh case is mlp_lib's at seed 0; the ReLU case follows the rule at the head of this file."""
    if case[3] != "ReLU":
        return M.inputs(case, 0), M.params(case, 0), 0, 0
    rows, D = case[0], sum(case[1])
    for seed in range(64):
        I, P = M.inputs(case, seed), M.params(case, seed)
        rng = np.random.RandomState(7000 + seed)
        redrawn = np.zeros(rows, bool)
        for _ in range(64):
            bad = np.flatnonzero(_row_margin(I["x"], P, case) < M.MARGIN)
            if len(bad) == 0:
                return I, P, int(redrawn.sum()), seed
            if rows > 2 and np.isin(bad, (1, 2)).any():
                break                                   # the constant or the zero row: these parameters will not do
            I["x"][bad] = rng.randn(len(bad), D).astype(np.float32)
            redrawn[bad] = True
    raise AssertionError("no parameter seed below 64 meets the ReLU margin for %s" % (case,))


def mlp_truth_of(case, I, P):
    """{array name: float64 value} over out_names: mlp_lib.truth64 for given inputs"""
    g = M.backward64(I["x"], P, I["gf"], case)
    out = dict(features=M.forward64(I["x"], P, case))
    for i, gp in enumerate(M.split(g.pop("grad_x"), case[1])):
        out["grad_part%d" % i] = gp
    out.update(g)
    return {k: out[k] for k in M.out_names(case)}


@functools.lru_cache(maxsize=None)
def mlp_truth(case):
    """(inputs, params, float64 truth) of one case"""
    I, P, _, _ = mlp_inputs(case)
    return I, P, mlp_truth_of(case, I, P)


@functools.lru_cache(maxsize=None)
def mlp_reference(case):
    """torch's float32 module stack on the CPU: the source of err_ref"""
    from test_gpu_mlp import torch_cpu_reference
    I, P, _ = mlp_truth(case)
    return torch_cpu_reference(case, I, P)


def mlp_margin(case):
    I, P, _, _ = mlp_inputs(case)
    return float(_row_margin(I["x"], P, case).min())


# ---------------------------------------------------------------------------------------------- GRU
@functools.lru_cache(maxsize=None)
def gru_truth(L, Nb, pattern):
    """(inputs, masks, params, float64 truth)"""
    return G.truth64(L, Nb, pattern)


@functools.lru_cache(maxsize=None)
def gru_reference(L, Nb, pattern):
    """torch's float32 nn.GRU + nn.LayerNorm on the CPU, step by step: the source of err_ref"""
    from test_gpu_gru import torch_cpu_reference
    I, m, P, _ = gru_truth(L, Nb, pattern)
    return torch_cpu_reference(I, m, P)
