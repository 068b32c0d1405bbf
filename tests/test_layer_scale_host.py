"""Host side of the GRU and MLPBase tests at the sizes where a workgroup owns several tiles (tests/layer_scale_lib.py, tests/test_gpu_layer_scale.py), no
GPU: the restated geometry gives exactly the workspace sizes of the C entries (which pins gmpe_wgrad::partition and the grid rules, since the number of
parts and k_mlp_bprop's grid enter the size); the restated constants are the sources'; every shape reaches the path it was chosen for; and the CPU float32
reference, from which the GPU tests take err_ref, stays under the cap against the float64 restatement at every accuracy case."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import abi_lib
import gmpe
import gru_lib as G
import layer_scale_lib as S
import mlp_lib as M
from gmpe import _lib

CSRC = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")


def test_partition_restated():
    assert S.partition(1) == (1, 1) and S.partition(32) == (1, 32) and S.partition(33) == (2, 17) and S.partition(4096) == (128, 32)
    assert S.partition(4097) == (128, 33) and S.partition(545) == (18, 31) and S.partition(512000) == (128, 4000)
    for M_ in (1, 31, 545, 4096, 4097, 4360, 8257, 16514, 32801):
        rng = S.part_ranges(M_)
        rows = [m for m0, m1 in rng for m in range(m0, m1)]
        assert rows == list(range(M_))                  # every row in exactly one part, in order


@pytest.mark.parametrize("rows,D,layer_n", S.MLP_SIZE_SHAPES)
def test_mlp_workspace_is_exactly_the_documented_layout(rows, D, layer_n):
    n = C.c_size_t(7)
    assert _lib.load().gmpe_mlp_workspace_bytes(rows, D, 64, layer_n, 1, C.byref(n)) == 0
    assert n.value == S.mlp_geometry(rows, D, layer_n)["workspace"] == gmpe.mlp_workspace_bytes(rows, D, layer_n)


@pytest.mark.parametrize("L,Nb", S.GRU_SIZE_SHAPES)
def test_gru_workspace_is_exactly_the_documented_layout(L, Nb):
    n = C.c_size_t(7)
    assert _lib.load().gmpe_gru_workspace_bytes(L, Nb, 64, 1, C.byref(n)) == 0
    assert n.value == S.gru_geometry(L, Nb)["workspace"] == gmpe.rnn_workspace_bytes(L, Nb, 64)


def test_the_restated_constants_are_the_sources():
    src = {f: open(os.path.join(CSRC, f)).read() for f in ("gmpe_host.h", "gmpe_wgrad.h")}

    def const(text, name):
        m = re.search(r"\b%s\s*=\s*([^,;]+)[,;]" % name, text)
        assert m, name
        return m.group(1).strip()
    assert int(const(src["gmpe_host.h"], "MAX_CU")) == S.MAX_CU == S.MAX_GRID         # the GRU's grids are the one rule's, at one workgroup per CU
    assert const(src["gmpe_host.h"], "LDS_CU") == "160 * 1024" and S.LDS_CU == 160 * 1024
    assert int(const(src["gmpe_wgrad.h"], "MAX_PARTS")) == S.MAX_PARTS and int(const(src["gmpe_wgrad.h"], "PART_ROWS")) == S.PART_ROWS
    assert const(src["gmpe_wgrad.h"], "FIN_SLICES") == "BLOCK / FIN_COLS"
    assert int(const(src["gmpe_wgrad.h"], "BLOCK")) // int(const(src["gmpe_wgrad.h"], "FIN_COLS")) == S.FIN_SLICES
    for name, mine, theirs in (("GMPE_MLP_ROW_TILE", S.MLP_TILE, M.TILE), ("GMPE_GRU_ROW_TILE", S.GRU_TILE, G.TILE)):
        assert abi_lib.constant(name) == mine == theirs, name
    assert S.H == M.H == G.H == G.D


@pytest.mark.parametrize("case", S.MLP_CASES, ids=M.key)
def test_every_mlp_shape_reaches_its_path(case):
    reach, g = S.mlp_reach(case), S.mlp_geometry_of(case)
    print(M.key(case), g, reach)
    assert S.MLP_REACH[case] and all(reach[k] for k in S.MLP_REACH[case]), reach


def test_the_mlp_shapes_in_numbers():
    g = {c[0]: S.mlp_geometry_of(c) for c in S.MLP_CASES}
    assert (g[545]["ntiles"], g[545]["grid_bwd"], g[545]["nparts"], g[545]["part_rows"]) == (18, 18, 18, 31)
    assert (g[4097]["nparts"], g[4097]["part_rows"], g[4097]["nblk1"]) == (128, 33, 2)
    assert [m0 >= 4097 for m0, _ in S.part_ranges(4097)] == [False] * 125 + [True] * 3           # parts 125 .. 127 hold no row
    assert (g[8257]["ntiles"], g[8257]["grid_fwd"], g[8257]["grid_bwd"], g[8257]["part_rows"]) == (259, 256, 256, 65)
    assert g[8257]["lds_fwd"] == max(S.mlp_geometry(1, D, n)["lds_fwd"] for D in (1, 29, 256) for n in (0, 1, 2)) <= S.LDS_CU
    assert (g[32801]["ntiles"], g[32801]["grid_fwd"], g[32801]["grid_bwd"], g[32801]["part_rows"]) == (1026, 1024, 256, 257)
    # what the training and rollout shapes of the kernels' notes run, and no smaller suite does
    big = S.mlp_reach((512000, (13, 16), 1, "ReLU", 1))
    assert big["loop_fwd"] and big["loop_bwd"] and big["slices"] and big["stages"]
    assert not any(S.mlp_reach((97, (67,), 2, "ReLU", 1)).values())


@pytest.mark.parametrize("L,Nb", S.GRU_CASES)
def test_every_gru_shape_reaches_its_path(L, Nb):
    reach, g = S.gru_reach(L, Nb), S.gru_geometry(L, Nb)
    print(L, Nb, g, reach)
    assert S.GRU_REACH[(L, Nb)] and all(reach[k] for k in S.GRU_REACH[(L, Nb)]), reach


def test_the_gru_shapes_in_numbers():
    g = {c: S.gru_geometry(*c) for c in S.GRU_CASES}
    assert (g[(8, 545)]["ntiles"], g[(8, 545)]["M"], g[(8, 545)]["part_rows"]) == (18, 4360, 35)
    assert (g[(17, 241)]["M"], g[(17, 241)]["nparts"], g[(17, 241)]["part_rows"]) == (4097, 128, 33)
    assert (g[(2, 8257)]["ntiles"], g[(2, 8257)]["grid"], g[(2, 8257)]["part_rows"]) == (259, 256, 130)
    small = S.gru_reach(10, 65)                         # the largest shape of tests/test_gpu_gru.py: parts of 31 rows across m = Nb, and nothing else
    assert [k for k, v in small.items() if v] == ["straddle"]


@pytest.mark.parametrize("case", S.MLP_CASES, ids=M.key)
def test_the_mlp_reference_stays_under_the_cap(case):
    I, P, t64 = S.mlp_truth(case)
    ref = S.mlp_reference(case)
    assert I["x"].shape == (case[0], sum(case[1])) and (I["x"][1] == 0.75).all() and (I["x"][2] == 0).all()
    for k in M.out_names(case):
        e = M.err(ref[k], t64[k])
        print("%s %-16s err_ref %.3g" % (M.key(case), k, e))
        assert ref[k].dtype == np.float32 and e < M.CAP, (case, k, e)
    if case[3] == "ReLU":
        _, _, redrawn, seed = S.mlp_inputs(case)
        margin = S.mlp_margin(case)
        print("%s parameter seed %d, %d rows redrawn, margin %.3g" % (M.key(case), seed, redrawn, margin))
        assert margin >= M.MARGIN and redrawn < 0.01 * case[0]


@pytest.mark.parametrize("L,Nb", S.GRU_CASES)
@pytest.mark.parametrize("pattern", S.GRU_PATTERNS)
def test_the_gru_reference_stays_under_the_cap(L, Nb, pattern):
    _, _, _, t64 = S.gru_truth(L, Nb, pattern)
    ref = S.gru_reference(L, Nb, pattern)
    for k, v in t64.items():
        e = G.err(ref[k], v)
        print("%s %-16s err_ref %.3g" % (G.key(L, Nb, pattern), k, e))
        assert ref[k].dtype == np.float32 and e < G.CAP, (L, Nb, pattern, k, e)


def test_the_exact_sum_inputs_are_what_they_claim():
    gf = S.integer_gf(32801)
    assert gf.dtype == np.float32 and set(np.unique(gf)) == {-2.0, -1.0, 0.0, 1.0, 2.0} and gf[3, 4] == (3 * 7 + 4) % 5 - 2
    assert np.abs(gf.astype(np.int64).sum(0)).max() < 2 ** 24             # the column sums are float32 integers
    assert not gf[8192:8257].sum(0).any()               # what the signed weights cannot see: 65 dropped rows
    pos = S.integer_gf(32801, 1)
    assert S.INTEGER_SHIFTS == (-2, 1) and pos.min() == 1 and pos.max() == 5 and pos.astype(np.int64).sum(0).max() < 2 ** 24
    oh = S.one_hot_gf(4097, 4096)
    assert np.flatnonzero(np.abs(oh).sum(1)).tolist() == [4096] and (oh[4096] != 0).all()
