// gmpe_head_rows.h — the action head's Linear for the row kernels (internal): one lane per row, the row's 64 features in registers, the weights in LDS
// read at wave-uniform addresses. One text for the dot product, so the forward entry (gmpe_head_forward) and the fused rollout entry (gmpe_act_head) of
// gmpe_head.hip give the same logits bit for bit:
//   logit[k] = fmaf chain from bias[k] over h = 0 .. 63 ascending of features[h] * weight[k][h].
// The files that include this compile with contraction off; the chain is explicit fmaf.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gmpe_host.h"            // TILE

namespace gmpe_head {

constexpr int H = 64;                                   // the one hidden size
constexpr int TILE = gmpe_ppo::TILE;
constexpr int FS = H + 4;                               // LDS row stride of a [TILE][64] tile in dwords: 16-byte units stay aligned, and the eight lanes of one
                                                        // ds_read_b128 / ds_write_b128 group, FS dwords apart, cover all banks once
constexpr int ROWS_LDS = TILE * FS;                     // floats of the rows region: a features tile, or (at stride S <= 65) a logits tile in its place

// the parameters [K][64] + [K] into LDS at w: weight rows back to back, then the bias
__device__ __forceinline__ void params_in(const float* __restrict__ weight, const float* __restrict__ bias, int K, bool vec, float* w) {
    const int n = K * H;
    if (vec)
        for (int f = threadIdx.x * 4; f < n; f += TILE * 4) *reinterpret_cast<float4*>(w + f) = *reinterpret_cast<const float4*>(weight + f);
    else
        for (int f = threadIdx.x; f < n; f += TILE) w[f] = weight[f];
    if (bias && (int)threadIdx.x < K) w[n + threadIdx.x] = bias[threadIdx.x];
}

// A contiguous tile of `rows` rows of 64 floats at g <-> the rows region at stride FS, coalesced: 16-byte units when vec (g 16-byte aligned), else dwords.
template <bool IN>
__device__ __forceinline__ void tile64_copy(float* g, float* sh, int rows, bool vec) {
    const int n = rows * H;
    if (vec) {
        for (int f = threadIdx.x * 4; f < n; f += TILE * 4) {
            float4* s = reinterpret_cast<float4*>(sh + (f >> 6) * FS + (f & 63));
            float4* q = reinterpret_cast<float4*>(g + f);
            if (IN) *s = *q; else *q = *s;
        }
    } else {
        for (int f = threadIdx.x; f < n; f += TILE) {
            float* s = sh + (f >> 6) * FS + (f & 63);
            if (IN) *s = g[f]; else g[f] = *s;
        }
    }
}

// this lane's row of the rows region -> registers (zeros for a lane without a row)
__device__ __forceinline__ void row_in(const float* sh, bool live, float (&x)[H]) {
    const float* my = sh + threadIdx.x * FS;
#pragma unroll
    for (int h = 0; h < H; h += 4) {
        const float4 v = live ? *reinterpret_cast<const float4*>(my + h) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        x[h] = v.x; x[h + 1] = v.y; x[h + 2] = v.z; x[h + 3] = v.w;
    }
}

// THE dot product: w = one weight row in LDS (a wave-uniform address: every read is a broadcast)
__device__ __forceinline__ float head_dot(const float (&x)[H], const float* __restrict__ w, float b) {
    float a = b;
#pragma unroll
    for (int h = 0; h < H; h += 4) {
        const float4 q = *reinterpret_cast<const float4*>(w + h);
        a = fmaf(x[h], q.x, a); a = fmaf(x[h + 1], q.y, a); a = fmaf(x[h + 2], q.z, a); a = fmaf(x[h + 3], q.w, a);
    }
    return a;
}

// The head of both kernels: the parameters and the tile's features come in, every lane takes its row into registers, and — behind a barrier, the features
// tile giving way — writes its K logits to `row`, its row of the logits tile at stride S in the same LDS. No barrier follows: a lane has written its own row only.
__device__ __forceinline__ void logits_rows(const float* feat_tile, int rows, bool live, bool vec_feat, const float* weight, const float* bias, bool vec_w, int K,
                                            float* sh, float* row) {
    float* w = sh + ROWS_LDS;
    params_in(weight, bias, K, vec_w, w);
    tile64_copy<true>(const_cast<float*>(feat_tile), sh, rows, vec_feat);
    __syncthreads();
    float x[H];
    row_in(sh, live, x);
    __syncthreads();
#pragma unroll 1
    for (int k = 0; k < K; ++k) row[k] = head_dot(x, w + k * H, w[K * H + k]);
}

static inline size_t lds_bytes(int K) { return (size_t)(ROWS_LDS + K * H + K) * sizeof(float); }
constexpr size_t LDS_MAX = (size_t)(ROWS_LDS + 64 * H + 64) * sizeof(float);

}  // namespace gmpe_head
