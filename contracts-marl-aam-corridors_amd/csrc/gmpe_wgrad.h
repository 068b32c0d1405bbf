// gmpe_wgrad.h — the parameter-gradient machinery the layer files share (gmpe_gru.hip, gmpe_mlp.hip, gmpe_head.hip, gmpe_value.hip; internal, nothing here has
// external linkage):
// gradients of 64-wide matrices and of per-column vectors as double sums in a fixed order, rounded to float32 once, without atomics.
//   weights: the M rows of a call are cut into P = min(128, ceil(M / 32)) contiguous parts of ceil(M / P) rows (partition). One workgroup adds a part's
//     exact double products a(m, j) * b(m, d) in ascending row order into a [64][64] block of doubles (part_products); the finish kernel adds the parts
//     in ascending part order (sum_parts).
//   columns: n partial rows of doubles are added as 16 interleaved slices (slice s: rows s, s + 16, ... ascending), then the slices in slice order
//     (sum_slices).
// So a sum's order is a function of M (and of n) alone.
// And the device pieces both files' kernels hold alike: the xor-tree sum over a wave, the float32 LayerNorm over the 64 columns a wave's lanes hold,
// forward and backward.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gmpe_wgrad {

constexpr int H = 64, BLOCK = 256;
constexpr int MAX_PARTS = 128, PART_ROWS = 32;          // parts, and rows per LDS stage
constexpr int FIN_COLS = 16, FIN_SLICES = BLOCK / FIN_COLS;

template <class T>
__device__ __forceinline__ T wave_sum(T v) {            // the same bits in every lane: a + b == b + a
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off);
    return v;
}

// LayerNorm over the 64 columns of a row, lane j holding column j's v: -> v - mean; the normalised value is that times rstd. Every operation is rounded
// on its own (the files compile with contraction off).
__device__ __forceinline__ float layer_norm_64(float v, float eps, float& mean, float& rstd) {
    mean = wave_sum(v) * (1.0f / H);
    const float d = v - mean;
    const float var = wave_sum(d * d) * (1.0f / H);
    rstd = __fdiv_rn(1.0f, __fsqrt_rn(var + eps));
    return d;
}

// ... and its backward: dxh = the output's gradient times the LayerNorm weight, xh the normalised value -> the gradient of v
__device__ __forceinline__ float layer_norm_64_backward(float dxh, float xh, float rstd) {
    const float s1 = wave_sum(dxh) * (1.0f / H), s2 = wave_sum(dxh * xh) * (1.0f / H);
    return rstd * ((dxh - s1) - xh * s2);
}

struct Parts { int nparts; int64_t part_rows; };
static inline Parts partition(int64_t M) {
    Parts y;
    const int64_t want = (M + PART_ROWS - 1) / PART_ROWS;
    y.nparts = (int)(want < MAX_PARTS ? want : MAX_PARTS);
    y.part_rows = (M + y.nparts - 1) / y.nparts;
    return y;
}

// out[j][d] = sum over m = m0 .. m1-1 ascending of a_of(m, j) * b_of(m, d), j, d = 0 .. 63, for a workgroup of BLOCK threads.
// Thread: j = tid / 4, d = 16 * (tid % 4) .. + 15. a_of / b_of (m, k): column k of row m < m1 of the two [rows][64] operands.
template <class LA, class LB>
__device__ __forceinline__ void part_products(int64_t m0, int64_t m1, LA a_of, LB b_of, double* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float As[PART_ROWS][H];
    __shared__ __attribute__((aligned(16))) float Bs[PART_ROWS][H];
    const int tid = threadIdx.x, j = tid >> 2, d0 = (tid & 3) * 16;
    double acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0;
    for (int64_t ms = m0; ms < m1; ms += PART_ROWS) {
        for (int i = tid; i < PART_ROWS * H; i += BLOCK) {
            const int mm = i >> 6, k = i & 63;
            const int64_t m = ms + mm;
            float a = 0.0f, b = 0.0f;
            if (m < m1) { a = a_of(m, k); b = b_of(m, k); }
            As[mm][k] = a; Bs[mm][k] = b;
        }
        __syncthreads();
#pragma unroll 2
        for (int mm = 0; mm < PART_ROWS; ++mm) {
            const double a = (double)As[mm][j];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 b = *reinterpret_cast<const float4*>(&Bs[mm][d0 + 4 * q]);
                acc[4 * q + 0] = fma(a, (double)b.x, acc[4 * q + 0]); acc[4 * q + 1] = fma(a, (double)b.y, acc[4 * q + 1]);
                acc[4 * q + 2] = fma(a, (double)b.z, acc[4 * q + 2]); acc[4 * q + 3] = fma(a, (double)b.w, acc[4 * q + 3]);
            }
        }
        __syncthreads();
    }
    double* o = out + j * H + d0;
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] = acc[i];
}

// element e of the parts' blocks (`stride` doubles from one part to the next), the parts in ascending order
__device__ __forceinline__ double sum_parts(const double* __restrict__ partW, int nparts, int64_t stride, int64_t e) {
    double s = 0.0;
    for (int q = 0; q < nparts; ++q) s += partW[(int64_t)q * stride + e];
    return s;
}

// Column `col0 + tid % 16` of the n rows of partC (ncol doubles each), for a workgroup of BLOCK threads: valid in the threads tid < 16 (slice 0); the other
// threads return 0 and have nothing to store. cs: FIN_SLICES * FIN_COLS doubles of LDS.
__device__ __forceinline__ double sum_slices(const double* __restrict__ partC, int64_t n, int ncol, int col0, double (*cs)[FIN_COLS]) {
    const int tid = threadIdx.x, jc = tid % FIN_COLS, s = tid / FIN_COLS, col = col0 + jc;
    double sum = 0.0;
    for (int64_t i = s; i < n; i += FIN_SLICES) sum += partC[i * ncol + col];
    cs[s][jc] = sum;
    __syncthreads();
    if (s != 0) return 0.0;
    double tot = cs[0][jc];
    for (int q = 1; q < FIN_SLICES; ++q) tot += cs[q][jc];
    return tot;
}

}  // namespace gmpe_wgrad
