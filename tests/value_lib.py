"""What the tests of the critic's value head share (include/gmpe.h gmpe_value_forward / gmpe_value_backward, gmpe.value_head): the seeded inputs, the
row counts, a NumPy float32 emulation of the forward's fixed order

    lane c of a row holds columns 4c .. 4c+3:  acc = 0.0f;  acc = acc + f[i] * w[i], i = 0 .. 3, multiply and add each rounded on its own;
    an xor tree over the 16 lanes, offsets 1, 2, 4, 8, the lower lane the left operand;  then + bias

a NumPy float64 emulation of the backward's fixed order of exact double products (emulate_backward), and the once-rounded truth of the backward's sums
(math.fsum over the exact double products, rounded to float32). Test infrastructure only."""
import functools
import math
import os

import numpy as np

H = 64
TILE = 256                      # rows per workgroup (csrc/gmpe_value.hip TILE)
COLS = 80                       # doubles per tile in the backward workspace: 64 weight columns, the bias column, padding
ROWS = (1, 63, 64, 65, 255, 256, 257, 1025)     # the edges of a wave, of a 256-row tile, and one row past four tiles
SLICES = 16                     # interleaved slices of tiles in the backward's finish (csrc/gmpe_wgrad.h FIN_SLICES)
MANY_ROWS = (4097, 8449)        # the smallest sizes at which a slice holds more than one tile: 17 tiles (slice 0 holds two), and 34 tiles (slices 0 and 1
                                # hold three, the others two) with one row in the last
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "policy_heads.npz")
f32 = np.float32


def workspace_bytes(rows):
    """the restated layout of gmpe_value_workspace_bytes: f64 [ceil(rows / 256)][80]"""
    return ((rows + TILE - 1) // TILE) * COLS * 8


@functools.lru_cache(maxsize=None)
def shipped():
    """(weight [1, 64], bias [1]) of the shipped critic's v_out"""
    with np.load(GOLDEN) as d:
        return d["critic.v_out.weight"].copy(), d["critic.v_out.bias"].copy()


@functools.lru_cache(maxsize=None)
def inputs(rows, source="random", positive_g=False):
    """(features ~ N(0, 1) [rows, 64] — what a LayerNorm hands over —, weight [1, 64], bias [1], grad_values [rows, 1]); float32, shared, never written to.
    positive_g: grad_values in (0.5, 1.5), so that the sum over the rows of g has no cancellation."""
    rng = np.random.RandomState(9100 + rows)
    f = rng.randn(rows, H).astype(f32)
    if source == "random":
        w, b = (rng.randn(1, H) / 8).astype(f32), (0.1 * rng.randn(1)).astype(f32)
    else:
        w, b = shipped()
    g = (rng.rand(rows, 1) + 0.5).astype(f32) if positive_g else rng.randn(rows, 1).astype(f32)
    for a in (f, w, b, g):
        a.setflags(write=False)
    return f, w, b, g


def emulate(f, w, b):
    """values [rows] float32 in the device's order; every operation is a float32 NumPy operation, so each is rounded on its own"""
    f, w, b = np.asarray(f, f32), np.asarray(w, f32).reshape(H), np.asarray(b, f32).reshape(())
    rows = f.shape[0]
    q = f.reshape(rows, 16, 4)
    wq = w.reshape(16, 4)
    acc = np.zeros((rows, 16), f32)
    for i in range(4):
        acc = acc + q[:, :, i] * wq[None, :, i]          # the product is rounded to float32 before the add
    for off in (1, 2, 4, 8):
        lanes = np.arange(16)
        other = acc[:, lanes ^ off]
        lower_left = np.where((lanes & off)[None, :] != 0, other + acc, acc + other)
        acc = lower_left.astype(f32)
    assert acc.dtype == f32 and (acc == acc[:, :1]).all()     # float32 addition commutes: every lane of a row ends with the same bits
    return (acc[:, 0] + b).astype(f32)


def emulate_backward(f, g, skip_tiles=()):
    """(grad_weight [1, 64], grad_bias [1]) float32 in the device's order, every add an IEEE double add of exact products:

        the exact double products g[r] * f[r, j] (and g[r] itself for the bias), rows past `rows` contributing 0.0;
        a lane over its 16 passes ascending, row = 256 * tile + 64 * wave + 4 * pass + sub;
        the wave's four row groups as (s0 + s1) + (s2 + s3);  the four waves in wave order;
        the tiles into 16 slices, slice i % 16, ascending inside a slice;  the slices in slice order;  one rounding to float32.

    skip_tiles: tiles left out of the slices — what a finish that loses them would give; for the tests of the inputs, not of the device."""
    f, g = np.asarray(f, f32), np.asarray(g, f32).reshape(-1)
    rows = f.shape[0]
    ntiles = (rows + TILE - 1) // TILE
    p = np.zeros((ntiles * TILE, H + 1), np.float64)
    p[:rows, :H] = g.astype(np.float64)[:, None] * f.astype(np.float64)     # exact: float32 x float32 fits a double
    p[:rows, H] = g
    p = p.reshape(ntiles, TILE // 64, 16, 4, H + 1)                          # tile, wave, pass, sub, column
    lane = np.zeros((ntiles, TILE // 64, 4, H + 1), np.float64)
    for ps in range(16):
        lane = lane + p[:, :, ps]
    wave = (lane[:, :, 0] + lane[:, :, 1]) + (lane[:, :, 2] + lane[:, :, 3])
    tile = wave[:, 0]
    for w in range(1, TILE // 64):
        tile = tile + wave[:, w]
    slices = np.zeros((SLICES, H + 1), np.float64)
    for i in range(ntiles):
        if i not in skip_tiles:
            slices[i % SLICES] = slices[i % SLICES] + tile[i]
    tot = slices[0]
    for q in range(1, SLICES):
        tot = tot + slices[q]
    out = tot.astype(f32)
    return out[:H].reshape(1, H).copy(), out[H:].reshape(1).copy()


def sum_abs(f, w):
    """sum over the columns of |f * w| per row, in float64: the scale of a row's rounding error"""
    return np.abs(np.asarray(f, np.float64) * np.asarray(w, np.float64).reshape(1, H)).sum(1)


def once_rounded(products):
    """float32(the exact sum) of float64 products that are themselves exact (float32 x float32), per column of [rows, n]"""
    p = np.asarray(products, np.float64)
    return np.array([f32(math.fsum(p[:, j])) for j in range(p.shape[1])], f32)


def neighbours(x):
    """[x - ulp, x, x + ulp] per element of a float32 array"""
    x = np.asarray(x, f32)
    return np.stack([np.nextafter(x, f32(-np.inf)), x, np.nextafter(x, f32(np.inf))])


def bits(a):
    return np.ascontiguousarray(np.asarray(a, f32)).reshape(-1).view(np.uint32)
