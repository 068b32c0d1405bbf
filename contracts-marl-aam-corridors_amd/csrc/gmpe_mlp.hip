// gmpe_mlp.hip — the policy's MLPBase, forward and backward (include/gmpe.h gmpe_mlp_forward / gmpe_mlp_backward): MLPBase.forward
// (onpolicy/algorithms/utils/mlp.py:44-76) over the columns of one to four parts read as if concatenated — optional LayerNorm(D), then 1 + layer_N times
// Linear -> ReLU | Tanh -> LayerNorm(64) — as ONE forward launch and THREE backward launches, whatever rows, D, layer_N and the number of parts.
//
// Mapping. A workgroup has four waves and owns tiles of GMPE_MLP_ROW_TILE = 32 rows, tile blockIdx.x, blockIdx.x + gridDim.x, ...; wave w owns rows
// 8w .. 8w+7 of the tile; lane j owns hidden column j of its wave's eight rows, and the input columns j, j + 64, j + 128, j + 192. The weights stand in LDS
// for the lifetime of the workgroup, transposed, [k][64] at row stride 65 dwords: forward reads a row across the lanes, backward (the product with W^T) reads
// element j of row `lane`, 65 dwords apart — both conflict-free. The dynamic LDS is sized by (D, layer_N): 7.5 KiB of W1 at D = 29, 65 KiB at D = 256.
// A wave's eight input rows are contiguous in every part, so a part is staged into the wave's own LDS by flat index (coalesced), the part boundaries
// resolved there and nowhere else; the vectors a chain multiplies with (the normalised input, a hidden layer's output, a layer's pre-activation gradient)
// are read from that LDS as broadcast 16-byte units, eight rows against one weight read. The part gradients leave the same way.
//
// The arithmetic of one row, a function of (D, layer_N, activation, feature_norm) alone — not of rows, of the row's place, of how the columns are split:
//   feature norm: its statistics in double — lane j adds its columns j, j + 64, ... ascending from 0; mean = xor-tree sum (offsets 32 .. 1) / D; var = the
//                 same sum of (x - mean)^2 / D; rstd = 1 / sqrt(var + eps); xh = float((x - mean) * rstd); xn = xh * w + b in float32. (A row of D = 2 or 3
//                 observations that lie close together next to their size loses in x - mean the digits a float32 mean does not have: 5e-7 in xh at the
//                 test shape D = 3, against 6e-8 with the statistics in double. The 64-wide LayerNorms behind an activation stay in float32.)
//   a layer, column j: a = fmaf chain from bias[j] over W[j][k] * in[k], k ascending (layer 1: k < D rounded up to 4, the padding being zeros);
//                 ReLU: a > 0 ? a : 0, or tanhf; LayerNorm as above over the 64 columns with / 64.
//   backward: LayerNorm backward dact = rstd * ((g * w - s1) - xh * s2), s1, s2 xor-tree means; dpre = dact where a > 0 (ReLU) or dact * (1 - a * a);
//                 the gradient of a layer's input column k = fmaf chain from 0 over W[j][k] * dpre[j], j ascending. Every other operation is rounded on its own.
// The backward launches recompute a tile's forward (the same code, the same bits) and keep nothing of the forward launch: the forward-only plan and the
// training plan run the same forward kernel.
//
// Parameter gradients, a fixed order that depends on (rows, D, layer_N) only (gmpe_wgrad.h, shared with gmpe_gru.hip):
//   biases, LayerNorm and feature-norm parameters: every lane adds its columns' terms in double over the tiles of its workgroup ascending and the rows of
//     its wave ascending; the four waves are added in wave order (k_mlp_bprop) into one row of doubles per workgroup; k_mlp_finish adds the workgroups as 16
//     interleaved slices, then the slices in slice order, and rounds to float32 once;
//   weights: the rows are cut into P = min(128, ceil(rows / 32)) contiguous parts; k_mlp_wgrad adds a part's exact double products in ascending row order,
//     one workgroup per part and 64-column block; k_mlp_finish adds the parts in ascending order and rounds to float32 once.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "gmpe_host.h"          // include/gmpe.h, the error text, GMPE_HIP_CHECK, the layer files' shared host half
#include "gmpe_wgrad.h"         // the weight-gradient parts, the ordered finish sums, wave_sum and the 64-wide LayerNorm, shared with gmpe_gru.hip

#pragma clang fp contract(off)

namespace {

constexpr int H = 64;                                   // the one hidden size
constexpr int TILE = GMPE_MLP_ROW_TILE, BLOCK = 256, NW = BLOCK / 64, R = TILE / NW;      // R rows per wave
constexpr int WS = H + 1;                               // row stride of the transposed weights in LDS
constexpr int MAXD = GMPE_MLP_MAX_IN, MAXL = GMPE_MLP_MAX_LAYERS, MAXP = GMPE_MLP_MAX_PARTS, NI = MAXD / 64;
constexpr int NQ = 3 * MAXL + 2 * NI;                   // column sums per lane: (bias, LayerNorm weight, bias) per layer, feature-norm weight and bias per 64 columns
constexpr int NCOL = NQ * H;                            // ... and per workgroup: column q * 64 + lane
using gmpe_wgrad::FIN_COLS;
using gmpe_wgrad::FIN_SLICES;
using gmpe_wgrad::wave_sum;
static_assert(R == 8 && TILE == NW * R && NI == 4 && MAXL == 3 && MAXP == 4, "eight rows per wave, four column groups, three layers, four parts");
static_assert(H == gmpe_wgrad::H && BLOCK == gmpe_wgrad::BLOCK, "gmpe_wgrad.h's workgroup");
constexpr size_t CS_LDS = (size_t)NW * NCOL * sizeof(double);

struct MlpArgs {
    int64_t rows, ntiles, part_rows;
    int D, DP, DS;                                      // input columns, rounded up to 4, and the row stride of a wave's LDS vectors: max(DP, 64)
    int nlayers, act, fnorm, nin, nparts, nblk1, nblocks;                // 1 + layer_N; parts of the input; wgrad parts; 64-column blocks of W1; k_mlp_bprop's grid
    const float* part[MAXP];
    float* gpart[MAXP];
    int pdim[MAXP], poff[MAXP];
    const float *fnw, *fnb;
    float fneps, eps[MAXL];
    const float *w[MAXL], *b[MAXL], *lw[MAXL], *lb[MAXL];
    float *gw[MAXL], *gb[MAXL], *glw[MAXL], *glb[MAXL], *gfnw, *gfnb;
    float* feat;
    const float* gf;
    float *dP, *Y;                                      // workspace: pre-activation gradients [nlayers][rows][64], layer outputs [layer_N][rows][64]
    double *S, *partC, *partW;                          // feature-norm mean / rstd [rows][2], [nblocks][NCOL], [nparts][nblk1 + layer_N][64][64]
};

template <class T>
__device__ __forceinline__ T pick(T const (&a)[MAXL], int i) { return i == 0 ? a[0] : (i == 1 ? a[1] : a[2]); }

__device__ __forceinline__ float activate(int act, float a) { return act == GMPE_MLP_RELU ? (a > 0.0f ? a : 0.0f) : tanhf(a); }

// what a lane keeps of the parameters: column `lane` of every layer, columns lane + 64 i of the feature norm
struct Lane {
    float b[MAXL], lw[MAXL], lb[MAXL], fw[NI], fb[NI];
};

__device__ __forceinline__ void load_lane(const MlpArgs& p, int lane, Lane& c) {
#pragma unroll
    for (int l = 0; l < MAXL; ++l) {
        c.b[l] = c.lw[l] = c.lb[l] = 0.0f;
        if (l < p.nlayers) { c.b[l] = p.b[l][lane]; c.lw[l] = p.lw[l][lane]; c.lb[l] = p.lb[l][lane]; }
    }
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int col = lane + 64 * i;
        const bool on = p.fnorm && col < p.D;
        c.fw[i] = on ? p.fnw[col] : 1.0f;
        c.fb[i] = on ? p.fnb[col] : 0.0f;
    }
}

// the weights into LDS, transposed: wt_l[k * WS + j] = W_l[j][k]; rows D .. DP-1 of layer 1 are zeros. -> floats used
__device__ __forceinline__ void load_weights(const MlpArgs& p, float* sh, int tid) {
    for (int i = tid; i < H * p.DP; i += BLOCK) {
        const int j = i / p.DP, k = i - j * p.DP;
        sh[k * WS + j] = k < p.D ? p.w[0][j * p.D + k] : 0.0f;
    }
#pragma unroll
    for (int l = 1; l < MAXL; ++l)
        if (l < p.nlayers) {
            float* wt = sh + p.DP * WS + (l - 1) * H * WS;
            for (int i = tid; i < H * H; i += BLOCK) wt[(i & 63) * WS + (i >> 6)] = p.w[l][i];
        }
}

__device__ __forceinline__ const float* weights_of(const MlpArgs& p, const float* sh, int l) { return l == 0 ? sh : sh + p.DP * WS + (l - 1) * H * WS; }

// acc[r] <- fmaf chain over k = 0 .. n-1 (n a multiple of 4) of wt[k][lane] * v[r][k]; v: the wave's [R][ds] broadcast vectors
__device__ __forceinline__ void chain_fwd(const float* __restrict__ wt, const float* __restrict__ v, int ds, int n, int lane, float (&acc)[R]) {
#pragma unroll 1
    for (int k = 0; k < n; k += 4) {
        float w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = wt[(k + i) * WS + lane];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float4 q = *reinterpret_cast<const float4*>(v + r * ds + k);
            float a = acc[r];
            a = fmaf(w[0], q.x, a); a = fmaf(w[1], q.y, a); a = fmaf(w[2], q.z, a); a = fmaf(w[3], q.w, a);
            acc[r] = a;
        }
    }
}

// acc[r] <- fmaf chain from 0 over j = 0 .. 63 of wt[row][j] * v[r][j]: column `row` of the product with W^T
__device__ __forceinline__ void chain_bwd(const float* __restrict__ wt, const float* __restrict__ v, int ds, int row, float (&acc)[R]) {
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.0f;
#pragma unroll 1
    for (int j = 0; j < H; j += 4) {
        float w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = wt[row * WS + j + i];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float4 q = *reinterpret_cast<const float4*>(v + r * ds + j);
            float a = acc[r];
            a = fmaf(w[0], q.x, a); a = fmaf(w[1], q.y, a); a = fmaf(w[2], q.z, a); a = fmaf(w[3], q.w, a);
            acc[r] = a;
        }
    }
}

// what backward keeps of a tile's forward, per lane
struct Kept {
    float a[MAXL][R], xh[MAXL][R], rs[MAXL][R];         // a layer's activation, its normalised value and rstd
    float x0h[NI][R], rs0[R];                           // the feature norm's normalised columns and rstd
};

// One tile's forward for a wave: rows row0 .. row0 + nvalid - 1 (the rest of the eight compute on zeros and store nothing). y: the last layer's output.
// Every wave of the workgroup calls it together (it holds workgroup barriers). KEEP: backward's copy, which also writes S and Y.
template <bool KEEP>
__device__ __forceinline__ void tile_forward(const MlpArgs& p, const Lane& c, const float* sh, float* st, int lane, int64_t row0, int nvalid, float (&y)[R], Kept* kp) {
    const int ds = p.DS;
#pragma unroll
    for (int q = 0; q < MAXP; ++q)
        if (q < p.nin) {                                // a part's eight rows are contiguous: flat index f = r * d + c
            const int d = p.pdim[q], n = nvalid * d;
            const float* src = p.part[q] + row0 * d;
            for (int f = lane; f < R * d; f += 64) {
                const int r = f / d, cc = f - r * d;
                st[r * ds + p.poff[q] + cc] = f < n ? src[f] : 0.0f;
            }
        }
    __syncthreads();
    const double Df = (double)p.D;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float xv[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int col = lane + 64 * i;
            xv[i] = col < p.D ? st[r * ds + col] : 0.0f;
        }
        if (p.fnorm) {                                  // the statistics in double: see the head of this file
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < NI; ++i) s = s + (double)xv[i];
            const double mean = wave_sum(s) / Df;
            double q = 0.0;
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const double d = (double)xv[i] - mean;
                q = q + (lane + 64 * i < p.D ? d * d : 0.0);
            }
            const double rstd = 1.0 / sqrt(wave_sum(q) / Df + (double)p.fneps);
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const float xh = lane + 64 * i < p.D ? (float)(((double)xv[i] - mean) * rstd) : 0.0f;
                if (KEEP) kp->x0h[i][r] = xh;
                xv[i] = xh * c.fw[i] + c.fb[i];
            }
            if (KEEP) {
                kp->rs0[r] = (float)rstd;
                if (lane == 0 && r < nvalid) { p.S[2 * (row0 + r)] = mean; p.S[2 * (row0 + r) + 1] = rstd; }
            }
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int col = lane + 64 * i;
            if (col < p.DP) st[r * ds + col] = col < p.D ? xv[i] : 0.0f;
        }
    }
    __syncthreads();
#pragma unroll
    for (int l = 0; l < MAXL; ++l)
        if (l < p.nlayers) {
            float acc[R];
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] = c.b[l];
            chain_fwd(weights_of(p, sh, l), st, ds, l == 0 ? p.DP : H, lane, acc);
            const bool more = l + 1 < p.nlayers;
            if (more) __syncthreads();                  // every wave has read its vectors: the layer's output takes their place
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float av = activate(p.act, acc[r]);
                float mean, rstd;
                const float xh = gmpe_wgrad::layer_norm_64(av, p.eps[l], mean, rstd) * rstd;
                y[r] = xh * c.lw[l] + c.lb[l];
                if (KEEP) { kp->a[l][r] = av; kp->xh[l][r] = xh; kp->rs[l][r] = rstd; }
                if (more) {
                    st[r * ds + lane] = y[r];
                    if (KEEP && r < nvalid) p.Y[((int64_t)l * p.rows + row0 + r) * H + lane] = y[r];
                }
            }
            if (more) __syncthreads();
        }
}

__global__ __launch_bounds__(BLOCK) void k_mlp_fwd(MlpArgs p) {
    extern __shared__ __attribute__((aligned(16))) float sh[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    float* st = sh + p.DP * WS + (p.nlayers - 1) * H * WS + wv * R * p.DS;          // this wave's vectors [R][DS]
    Lane c;
    load_lane(p, lane, c);
    load_weights(p, sh, tid);
    __syncthreads();
    for (int64_t tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
        const int64_t row0 = tile * TILE + wv * R;
        const int64_t left = p.rows - row0;
        const int nvalid = left >= R ? R : (left > 0 ? (int)left : 0);
        float y[R];
        tile_forward<false>(p, c, sh, st, lane, row0, nvalid, y, nullptr);
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (r < nvalid) p.feat[(row0 + r) * H + lane] = y[r];
        __syncthreads();                                // the next tile overwrites the waves' vectors
    }
}

// backward 1: a tile's forward again, then back through the layers (the head of this file)
__global__ __launch_bounds__(BLOCK) void k_mlp_bprop(MlpArgs p) {
    extern __shared__ __attribute__((aligned(16))) float sh[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, ds = p.DS;
    float* st = sh + p.DP * WS + (p.nlayers - 1) * H * WS + wv * R * ds;
    Lane c;
    load_lane(p, lane, c);
    load_weights(p, sh, tid);
    __syncthreads();
    double cq[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) cq[q] = 0.0;
    for (int64_t tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
        const int64_t row0 = tile * TILE + wv * R;
        const int64_t left = p.rows - row0;
        const int nvalid = left >= R ? R : (left > 0 ? (int)left : 0);
        float dy[R];
        Kept kp;
        tile_forward<true>(p, c, sh, st, lane, row0, nvalid, dy, &kp);
#pragma unroll
        for (int r = 0; r < R; ++r) dy[r] = r < nvalid ? p.gf[(row0 + r) * H + lane] : 0.0f;
        float dxn[NI][R];
#pragma unroll
        for (int l = MAXL - 1; l >= 0; --l)
            if (l < p.nlayers) {
                float dp[R];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const float g = dy[r], xh = kp.xh[l][r], av = kp.a[l][r];
                    const float dxh = g * c.lw[l];
                    const float dact = gmpe_wgrad::layer_norm_64_backward(dxh, xh, kp.rs[l][r]);
                    dp[r] = p.act == GMPE_MLP_RELU ? (av > 0.0f ? dact : 0.0f) : dact * (1.0f - av * av);
                    if (r < nvalid) {
                        cq[3 * l] += (double)dp[r]; cq[3 * l + 1] += (double)g * (double)xh; cq[3 * l + 2] += (double)g;
                        p.dP[((int64_t)l * p.rows + row0 + r) * H + lane] = dp[r];
                    }
                }
                __syncthreads();                        // the vectors the last chains read give way to this layer's pre-activation gradients
#pragma unroll
                for (int r = 0; r < R; ++r) st[r * ds + lane] = dp[r];
                __syncthreads();
                const float* wt = weights_of(p, sh, l);
                if (l > 0) chain_bwd(wt, st, ds, lane, dy);
                else {
#pragma unroll
                    for (int i = 0; i < NI; ++i) {
#pragma unroll
                        for (int r = 0; r < R; ++r) dxn[i][r] = 0.0f;
                        if (64 * i < p.D) {
                            const int col = lane + 64 * i;
                            chain_bwd(wt, st, ds, col < p.DP ? col : p.DP - 1, dxn[i]);
                        }
                    }
                }
            }
        __syncthreads();                                // the pre-activation gradients give way to the input gradients
        const float Df = (float)p.D;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float dx[NI];
            if (p.fnorm) {
                float s1 = 0.0f, s2 = 0.0f, dxh[NI];
#pragma unroll
                for (int i = 0; i < NI; ++i) {
                    const bool on = lane + 64 * i < p.D;
                    dxh[i] = on ? dxn[i][r] * c.fw[i] : 0.0f;
                    s1 = s1 + dxh[i];
                    s2 = s2 + dxh[i] * kp.x0h[i][r];
                    if (on && r < nvalid) { cq[3 * MAXL + i] += (double)dxn[i][r] * (double)kp.x0h[i][r]; cq[3 * MAXL + NI + i] += (double)dxn[i][r]; }
                }
                s1 = __fdiv_rn(wave_sum(s1), Df); s2 = __fdiv_rn(wave_sum(s2), Df);
#pragma unroll
                for (int i = 0; i < NI; ++i) dx[i] = kp.rs0[r] * ((dxh[i] - s1) - kp.x0h[i][r] * s2);
            } else {
#pragma unroll
                for (int i = 0; i < NI; ++i) dx[i] = dxn[i][r];
            }
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int col = lane + 64 * i;
                if (col < p.D) st[r * ds + col] = dx[i];
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < MAXP; ++q)
            if (q < p.nin) {
                const int d = p.pdim[q], n = nvalid * d;
                float* dst = p.gpart[q] + row0 * d;
                for (int f = lane; f < n; f += 64) {
                    const int r = f / d, cc = f - r * d;
                    dst[f] = st[r * ds + p.poff[q] + cc];
                }
            }
        __syncthreads();                                // the next tile overwrites the waves' vectors
    }
    double* cs = reinterpret_cast<double*>(sh);         // [NW][NCOL] over the weights, which nothing reads any more
#pragma unroll
    for (int q = 0; q < NQ; ++q) cs[wv * NCOL + q * H + lane] = cq[q];
    __syncthreads();
    for (int i = tid; i < NCOL; i += BLOCK) {
        double s = cs[i];
        for (int w = 1; w < NW; ++w) s += cs[w * NCOL + i];
        p.partC[(int64_t)blockIdx.x * NCOL + i] = s;
    }
}

// column `col` of the (concatenated, normalised) input of row m, with forward's roundings
__device__ __forceinline__ float input_of(const MlpArgs& p, int64_t m, int col) {
    if (col >= p.D) return 0.0f;
    float v = 0.0f;
#pragma unroll
    for (int q = 0; q < MAXP; ++q)
        if (q < p.nin && col >= p.poff[q] && col < p.poff[q] + p.pdim[q]) v = p.part[q][m * p.pdim[q] + (col - p.poff[q])];
    if (p.fnorm) v = (float)(((double)v - p.S[2 * m]) * p.S[2 * m + 1]) * p.fnw[col] + p.fnb[col];
    return v;
}

// backward 2: part blockIdx.x of the rows, block blockIdx.y: 0 .. nblk1-1 columns 64 y .. 64 y + 63 of W1, then the hidden layers' matrices
__global__ __launch_bounds__(BLOCK) void k_mlp_wgrad(MlpArgs p) {
    const int y = blockIdx.y, l = y < p.nblk1 ? 0 : y - p.nblk1 + 1, nmat = p.nblk1 + p.nlayers - 1;
    const int64_t m0 = (int64_t)blockIdx.x * p.part_rows, m1 = m0 + p.part_rows < p.rows ? m0 + p.part_rows : p.rows;
    const float* dP = p.dP + (int64_t)l * p.rows * H;
    const float* Y = p.Y + (int64_t)(l - 1) * p.rows * H;
    gmpe_wgrad::part_products(
        m0, m1, [&](int64_t m, int k) { return dP[m * H + k]; },
        [&](int64_t m, int k) { return l == 0 ? input_of(p, m, 64 * y + k) : Y[m * H + k]; },
        p.partW + ((int64_t)blockIdx.x * nmat + y) * H * H);
}

// backward 3: the partial sums in their fixed order, rounded once. Workgroups 0 .. 16 nmat - 1: one weight element per thread; then 16 columns of partC each.
__global__ __launch_bounds__(BLOCK) void k_mlp_finish(MlpArgs p) {
    __shared__ double cs[FIN_SLICES][FIN_COLS];
    const int tid = threadIdx.x, nmat = p.nblk1 + p.nlayers - 1, wblocks = nmat * (H * H / BLOCK);
    if ((int)blockIdx.x < wblocks) {
        const int e = blockIdx.x * BLOCK + tid, y = e >> 12, j = (e >> 6) & 63, d = e & 63;
        const float v = (float)gmpe_wgrad::sum_parts(p.partW, p.nparts, (int64_t)nmat * H * H, e);
        if (y < p.nblk1) {
            if (64 * y + d < p.D) p.gw[0][j * p.D + 64 * y + d] = v;
        } else
            pick(p.gw, y - p.nblk1 + 1)[j * H + d] = v;
        return;
    }
    const int col0 = ((int)blockIdx.x - wblocks) * FIN_COLS;
    const double tot = gmpe_wgrad::sum_slices(p.partC, p.nblocks, NCOL, col0, cs);
    if (tid >= FIN_COLS) return;
    const float v = (float)tot;
    const int col = col0 + tid, q = col / H, jj = col % H;
    if (q < 3 * MAXL) {
        const int l = q / 3, kind = q % 3;
        if (l < p.nlayers) pick(kind == 0 ? p.gb : (kind == 1 ? p.glw : p.glb), l)[jj] = v;
    } else if (p.fnorm) {
        const int i = q - 3 * MAXL, cc = 64 * (i % NI) + jj;
        if (cc < p.D) (i < NI ? p.gfnw : p.gfnb)[cc] = v;
    }
}

using gmpe::fail;

struct Layout {
    size_t partC, partW, dP, Y, S, total;
    int64_t ntiles, part_rows;
    int nparts, nblk1, DP, DS, nblocks_fwd, nblocks_bwd;
    size_t lds_fwd, lds_bwd;
};

bool layout(int64_t rows, int D, int layer_n, Layout& y) {
    if (rows < 1 || rows > (int64_t)1 << 40 || D < 1 || D > MAXD || layer_n < 0 || layer_n >= MAXL) return false;
    y.ntiles = (rows + TILE - 1) / TILE;
    const gmpe_wgrad::Parts parts = gmpe_wgrad::partition(rows);
    y.nparts = parts.nparts; y.part_rows = parts.part_rows;
    y.nblk1 = (D + 63) / 64;
    y.DP = (D + 3) & ~3;
    y.DS = y.DP > H ? y.DP : H;
    y.lds_fwd = (size_t)(y.DP * WS + layer_n * H * WS + NW * R * y.DS) * sizeof(float);
    y.lds_bwd = y.lds_fwd > CS_LDS ? y.lds_fwd : CS_LDS;
    y.nblocks_fwd = gmpe::resident_grid(y.ntiles, y.lds_fwd, 4);
    y.nblocks_bwd = gmpe::resident_grid(y.ntiles, y.lds_bwd, 1);           // k_mlp_bprop keeps a tile's forward in registers: one wave per SIMD
    gmpe::Carver c;
    y.partC = c.take((size_t)y.nblocks_bwd * NCOL * sizeof(double));
    y.partW = c.take((size_t)y.nparts * (y.nblk1 + layer_n) * H * H * sizeof(double));
    y.S = c.take((size_t)rows * 2 * sizeof(double));
    y.dP = c.take((size_t)rows * (layer_n + 1) * H * sizeof(float));
    y.Y = c.take((size_t)rows * layer_n * H * sizeof(float));
    y.total = c.total();
    return true;
}

// the checks both entry points make alike, before any device call
int check_plan(const char* fn, const gmpe_mlp_plan* pl, bool backward, Layout& y, int& D) {
    if (!pl) return fail(fn, "null plan");
    if (pl->rows < 1) return fail(fn, "rows must be >= 1");
    if (pl->hidden != H) return fail(fn, "unsupported hidden = " + std::to_string(pl->hidden) + ": only 64 is built");
    if (pl->layer_n < 0 || pl->layer_n >= MAXL) return fail(fn, "unsupported layer_n = " + std::to_string(pl->layer_n) + ": 0 .. 2 are built");
    if (pl->activation != GMPE_MLP_RELU && pl->activation != GMPE_MLP_TANH) return fail(fn, "activation must be GMPE_MLP_RELU or GMPE_MLP_TANH");
    if (pl->feature_norm != 0 && pl->feature_norm != 1) return fail(fn, "feature_norm must be 0 or 1");
    if (pl->n_parts < 1 || pl->n_parts > MAXP) return fail(fn, "n_parts must be in 1 .. " + std::to_string(MAXP));
    D = 0;
    for (int q = 0; q < pl->n_parts; ++q) {
        const std::string name = "[" + std::to_string(q) + "]";
        if (pl->part_dim[q] < 1 || pl->part_dim[q] > MAXD) return fail(fn, "part_dim" + name + " must be in 1 .. " + std::to_string(MAXD));
        D += pl->part_dim[q];
        if (!pl->part[q]) return fail(fn, "part" + name + " is required");
        if ((uintptr_t)pl->part[q] & 3) return fail(fn, "part" + name + " must be 4-byte aligned");
        if (backward && !pl->grad_part[q]) return fail(fn, "grad_part" + name + " is required");
        if ((uintptr_t)pl->grad_part[q] & 3) return fail(fn, "grad_part" + name + " must be 4-byte aligned");
    }
    if (D > MAXD) return fail(fn, "unsupported sum of part_dim = " + std::to_string(D) + ": at most " + std::to_string(MAXD) + " input columns are built");
    if (!layout(pl->rows, D, pl->layer_n, y)) return fail(fn, "rows is too large");
    if (y.ntiles > 0x7fffffffLL) return fail(fn, "rows: too many for one launch");
    if (pl->feature_norm) {
        if (!(pl->fn_eps > 0.0)) return fail(fn, "fn_eps must be > 0");
        const gmpe::PtrField ps[] = {
            {pl->fn_weight, "fn_weight", true}, {pl->fn_bias, "fn_bias", true}, {pl->grad_fn_weight, "grad_fn_weight", backward},
            {pl->grad_fn_bias, "grad_fn_bias", backward}};
        if (int rc = gmpe::check_ptrs(fn, ps)) return rc;
    }
    for (int l = 0; l <= pl->layer_n; ++l) {
        const gmpe_mlp_layer& L = pl->layer[l];
        const std::string n = "layer[" + std::to_string(l) + "].";
        if (!(L.eps > 0.0)) return fail(fn, n + "eps must be > 0");
        const gmpe::PtrField ps[] = {
            {L.weight, "weight", true}, {L.bias, "bias", true}, {L.ln_weight, "ln_weight", true}, {L.ln_bias, "ln_bias", true},
            {L.grad_weight, "grad_weight", backward}, {L.grad_bias, "grad_bias", backward}, {L.grad_ln_weight, "grad_ln_weight", backward},
            {L.grad_ln_bias, "grad_ln_bias", backward}};
        if (int rc = gmpe::check_ptrs(fn, ps, n)) return rc;
    }
    if (int rc = gmpe::check_ptr(fn, pl->features, "features", !backward)) return rc;
    if (int rc = gmpe::check_ptr(fn, pl->grad_features, "grad_features", backward)) return rc;
    return gmpe::check_workspace(fn, pl->workspace, pl->workspace_bytes, y.total, backward, "workspace is required",
                                 "gmpe_mlp_workspace_bytes(rows, in_dim, hidden, layer_n, 1)");
}

MlpArgs bind(const gmpe_mlp_plan* pl, const Layout& y, int D) {
    MlpArgs a = {};
    a.rows = pl->rows; a.ntiles = y.ntiles; a.part_rows = y.part_rows;
    a.D = D; a.DP = y.DP; a.DS = y.DS;
    a.nlayers = pl->layer_n + 1; a.act = pl->activation; a.fnorm = pl->feature_norm; a.nin = pl->n_parts; a.nparts = y.nparts; a.nblk1 = y.nblk1;
    a.nblocks = y.nblocks_bwd;
    int off = 0;
    for (int q = 0; q < pl->n_parts; ++q) {
        a.part[q] = pl->part[q]; a.gpart[q] = pl->grad_part[q]; a.pdim[q] = pl->part_dim[q]; a.poff[q] = off;
        off += pl->part_dim[q];
    }
    if (pl->feature_norm) {
        a.fnw = pl->fn_weight; a.fnb = pl->fn_bias; a.fneps = (float)pl->fn_eps; a.gfnw = pl->grad_fn_weight; a.gfnb = pl->grad_fn_bias;
    }
    for (int l = 0; l < a.nlayers; ++l) {
        const gmpe_mlp_layer& L = pl->layer[l];
        a.w[l] = L.weight; a.b[l] = L.bias; a.lw[l] = L.ln_weight; a.lb[l] = L.ln_bias; a.eps[l] = (float)L.eps;
        a.gw[l] = L.grad_weight; a.gb[l] = L.grad_bias; a.glw[l] = L.grad_ln_weight; a.glb[l] = L.grad_ln_bias;
    }
    a.feat = pl->features; a.gf = pl->grad_features;
    void* w = pl->workspace;
    a.dP = gmpe::at<float>(w, y.dP); a.Y = gmpe::at<float>(w, y.Y); a.S = gmpe::at<double>(w, y.S);
    a.partC = gmpe::at<double>(w, y.partC); a.partW = gmpe::at<double>(w, y.partW);
    return a;
}

}  // namespace

extern "C" {

int gmpe_mlp_workspace_bytes(int64_t rows, int32_t in_dim, int32_t hidden, int32_t layer_n, int32_t want_backward, size_t* bytes_out) {
    const char* fn = "gmpe_mlp_workspace_bytes";
    Layout y;
    const auto dims = [&]() -> std::string {
        if (hidden != H) return "unsupported hidden = " + std::to_string(hidden) + ": only 64 is built";
        if (layer_n < 0 || layer_n >= MAXL) return "unsupported layer_n = " + std::to_string(layer_n) + ": 0 .. 2 are built";
        if (in_dim < 1 || in_dim > MAXD) return "in_dim must be in 1 .. " + std::to_string(MAXD);
        return std::string();
    };
    if (int rc = gmpe::check_workspace_query(fn, bytes_out, dims(), want_backward)) return rc;
    if (!layout(rows, in_dim, layer_n, y)) return fail(fn, "rows must be >= 1 (and not absurd)");
    *bytes_out = want_backward ? y.total : 0;
    return GMPE_OK;
}

int gmpe_mlp_forward(int device, const gmpe_mlp_plan* pl, void* stream) {
    Layout y;
    int D;
    if (int rc = check_plan("gmpe_mlp_forward", pl, false, y, D)) return rc;
    GMPE_HIP_CHECK(hipSetDevice(device));
    if (int rc = gmpe::raise_dynamic_lds_once(reinterpret_cast<const void*>(k_mlp_fwd), device, 0, gmpe::LDS_CU)) return rc;
    const MlpArgs a = bind(pl, y, D);
    GMPE_LAUNCH(k_mlp_fwd, dim3((unsigned)y.nblocks_fwd), dim3(BLOCK), y.lds_fwd, static_cast<hipStream_t>(stream), a);
    return GMPE_OK;
}

int gmpe_mlp_backward(int device, const gmpe_mlp_plan* pl, void* stream) {
    Layout y;
    int D;
    if (int rc = check_plan("gmpe_mlp_backward", pl, true, y, D)) return rc;
    GMPE_HIP_CHECK(hipSetDevice(device));
    if (int rc = gmpe::raise_dynamic_lds_once(reinterpret_cast<const void*>(k_mlp_bprop), device, 1, gmpe::LDS_CU)) return rc;
    const MlpArgs a = bind(pl, y, D);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nmat = y.nblk1 + pl->layer_n;
    GMPE_LAUNCH(k_mlp_bprop, dim3((unsigned)y.nblocks_bwd), dim3(BLOCK), y.lds_bwd, st, a);
    GMPE_LAUNCH(k_mlp_wgrad, dim3((unsigned)y.nparts, (unsigned)nmat), dim3(BLOCK), 0, st, a);
    GMPE_LAUNCH(k_mlp_finish, dim3((unsigned)(nmat * (H * H / BLOCK) + NCOL / FIN_COLS)), dim3(BLOCK), 0, st, a);
    return GMPE_OK;
}

}  // extern "C"
