// gmpe_gru.hip — the policy's masked GRU layer, forward and backward (include/gmpe.h gmpe_gru_forward / gmpe_gru_backward): RNNLayer.forward
// (onpolicy/algorithms/utils/rnn.py:23-79) with recurrent_N == 1 and D = H = 64, as ONE forward launch and THREE backward launches, whatever the
// number of steps L, of rows Nb and the masks (the reference synchronises with the host to find the zero masks and loops over the segments).
//
// Mapping (forward and back-propagation through time alike). A workgroup has four waves and owns tiles of GMPE_GRU_ROW_TILE = 32 rows, tile
// blockIdx.x, blockIdx.x + gridDim.x, ...; wave w owns rows 8w .. 8w+7 of the tile for all L steps; lane j owns column j (of h, of every gate, of x
// and of features) of its wave's eight rows. Both weight matrices (96 KiB) stand in LDS for the lifetime of the workgroup, read once per workgroup:
//   forward:  transposed, [k][3H] at row stride 193 dwords (the transposing stores and the lane-consecutive reads are both conflict-free);
//   backward: as they are, [3H][64] (the products with W^T read a row across the lanes).
// The vectors a chain multiplies with (x_t and h of a row; the four gate gradients of a row) go through a wave's own 2 / 8 KiB of LDS and are read as
// broadcast 16-byte units, eight rows against one weight read.
//
// The arithmetic of one row, a function of (D, H) alone:
//   forward, column j:  a_r = fmaf chain from (b_ir[j] + b_hr[j]) over W_ir[j][k] x[k], k = 0 .. 63, then over W_hr[j][k] h[k], k = 0 .. 63; a_z alike;
//                       a_in from b_in[j] over x; a_hn from b_hn[j] over h; r = 1 / (1 + expf(-a_r)), z alike, n = tanhf(a_in + r * a_hn),
//                       h' = (1 - z) * n + z * h, every operation rounded on its own (no contraction outside the chains);
//                       LayerNorm: mean = xor-tree sum (offsets 32 .. 1) / 64, var = xor-tree sum of (h' - mean)^2 / 64, rstd = 1 / sqrt(var + eps).
//   backward, column j: dh_t = dh (from t+1) + LayerNorm backward; the gate gradients; grad_x[j] = fmaf chain from 0 over W_i?[i][j] * d?[i] for the
//                       gates r, z, n in this order, i = 0 .. 63 inside a gate; the state gradient the same over W_h? (dhn for its n gate), + dh_t * z last — the
//                       chain's terms are small next to dh_t * z, which would cost every one of them a rounding at its size —, times masks[t].
// This is the order of a k-ascending fmaf chain, which is also what mfma_f32_32x32x2f32 computes; these kernels use the vector unit.
//
// Parameter gradients, a fixed order that depends on (L, Nb) only:
//   biases and LayerNorm: every lane adds its column's terms in double, t descending and inside a step the rows of its wave ascending; the four waves of
//     a tile are added in wave order (k_gru_bptt) into one row of 6 * 64 doubles per tile; k_gru_finish adds the tiles as 16 interleaved slices (slice s:
//     tiles s, s + 16, ... ascending), then the slices in slice order, and rounds to float32 once;
//   weights: the M = L * Nb time-major rows are cut into P = min(128, ceil(M / 32)) contiguous parts of ceil(M / P) rows; k_gru_wgrad adds a part's
//     exact double products in ascending row order; k_gru_finish adds the parts in ascending part order and rounds to float32 once.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "gmpe_host.h"          // include/gmpe.h, the error text, GMPE_HIP_CHECK, the layer files' shared host half
#include "gmpe_wgrad.h"         // the weight-gradient parts, the ordered finish sums, wave_sum and the 64-wide LayerNorm, shared with gmpe_mlp.hip

#pragma clang fp contract(off)

namespace {

constexpr int H = 64;                                   // = D: the one instantiation
constexpr int G3 = 3 * H, G4 = 4 * H;
constexpr int TILE = GMPE_GRU_ROW_TILE, BLOCK = 256, NW = BLOCK / 64, R = TILE / NW;     // R rows per wave
constexpr int WS = G3 + 1;                              // row stride of the transposed weights in LDS
constexpr int NCOL = 6 * H;                             // dr, dz, dn, dhn (the bias gradients), LayerNorm weight, bias
using gmpe_wgrad::FIN_COLS;                             // k_gru_wgrad's parts and k_gru_finish's slices: gmpe_wgrad.h
using gmpe_wgrad::FIN_SLICES;
static_assert(H == gmpe_wgrad::H && BLOCK == gmpe_wgrad::BLOCK, "gmpe_wgrad.h's workgroup");
static_assert(R == 8 && TILE == NW * R, "eight rows per wave");
constexpr size_t FWD_LDS = (size_t)(2 * H * WS + 2 * NW * R * H) * sizeof(float);
constexpr size_t BPTT_LDS = (size_t)(2 * G3 * H + NW * R * G4) * sizeof(float) + (size_t)NW * NCOL * sizeof(double);
static_assert((2 * H * WS) % 4 == 0, "the broadcast vectors start at a 16-byte boundary");
static_assert(FWD_LDS <= gmpe::LDS_CU && BPTT_LDS <= gmpe::LDS_CU, "one workgroup's LDS");      // one per CU fits; tiles beyond that are looped over

struct GruArgs {
    int64_t L, Nb, M, ntiles, part_rows;
    int nparts;
    float eps;
    const float *x, *hxs, *masks, *wih, *whh, *bih, *bhh, *lnw, *lnb;
    float *feat, *hout;
    float *sG, *sH, *sS, *dG;                           // workspace: gates [M, 4H], h [M, H], mean / rstd [M, 2], gate gradients [M, 4H]
    double *partC, *partW;                              // [ntiles, 6H], [nparts, 6, H, H]
    const float *gf, *gho;
    float *gx, *ghxs, *gwih, *gwhh, *gbih, *gbhh, *glnw, *glnb;
};

__device__ __forceinline__ float sigmoid(float a) { return __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-a))); }

// acc[r] <- fmaf chain over k = 0 .. 63 of wt[k][c0 + lane] * v[r][k] for NG gate columns; v: the wave's [R][64] broadcast vectors
template <int NG>
__device__ __forceinline__ void chains_fwd(const float* __restrict__ wt, const float* __restrict__ v, int lane, float (&acc)[NG][R]) {
#pragma unroll 1
    for (int k = 0; k < H; k += 4) {
        float w[4][NG];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int g = 0; g < NG; ++g) w[i][g] = wt[(k + i) * WS + g * H + lane];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float4 q = *reinterpret_cast<const float4*>(v + r * H + k);
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                float a = acc[g][r];
                a = fmaf(w[0][g], q.x, a); a = fmaf(w[1][g], q.y, a); a = fmaf(w[2][g], q.z, a); a = fmaf(w[3][g], q.w, a);
                acc[g][r] = a;
            }
        }
    }
}

template <bool SAVE>
__global__ __launch_bounds__(BLOCK) void k_gru_fwd(GruArgs p) {
    extern __shared__ __attribute__((aligned(16))) float sh[];
    float* wt_ih = sh;                                  // [64][WS]: wt[k][g * 64 + j] = W[g * 64 + j][k]
    float* wt_hh = sh + H * WS;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    float* xw = sh + 2 * H * WS + wv * R * H;           // this wave's x_t [R][64]
    float* hw = sh + 2 * H * WS + NW * R * H + wv * R * H;          // and its masked h [R][64]
    for (int i = tid; i < G3 * H; i += BLOCK) {
        const int row = i >> 6, k = i & 63;
        wt_ih[k * WS + row] = p.wih[i];
        wt_hh[k * WS + row] = p.whh[i];
    }
    const float b_r = __fadd_rn(p.bih[lane], p.bhh[lane]), b_z = __fadd_rn(p.bih[H + lane], p.bhh[H + lane]);
    const float b_in = p.bih[2 * H + lane], b_hn = p.bhh[2 * H + lane], lw = p.lnw[lane], lb = p.lnb[lane];
    __syncthreads();
    for (int64_t tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
        const int64_t row0 = tile * TILE + wv * R;
        float h[R];
#pragma unroll
        for (int r = 0; r < R; ++r) h[r] = row0 + r < p.Nb ? p.hxs[(row0 + r) * H + lane] : 0.0f;
        for (int64_t t = 0; t < p.L; ++t) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const bool ok = row0 + r < p.Nb;
                const int64_t m = t * p.Nb + row0 + r;
                h[r] = __fmul_rn(h[r], ok ? p.masks[m] : 0.0f);
                xw[r * H + lane] = ok ? p.x[m * H + lane] : 0.0f;
                hw[r * H + lane] = h[r];
            }
            __syncthreads();
            float a3[3][R], a1[1][R];                   // r, z, W_in x + b_in; W_hn h + b_hn
#pragma unroll
            for (int r = 0; r < R; ++r) { a3[0][r] = b_r; a3[1][r] = b_z; a3[2][r] = b_in; a1[0][r] = b_hn; }
            chains_fwd<3>(wt_ih, xw, lane, a3);
            float a2[2][R];
#pragma unroll
            for (int r = 0; r < R; ++r) { a2[0][r] = a3[0][r]; a2[1][r] = a3[1][r]; }
            chains_fwd<2>(wt_hh, hw, lane, a2);
            chains_fwd<1>(wt_hh + 2 * H, hw, lane, a1);
            __syncthreads();                            // the next step (or tile) overwrites xw / hw
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const bool ok = row0 + r < p.Nb;
                const int64_t m = t * p.Nb + row0 + r;
                const float rr = sigmoid(a2[0][r]), zz = sigmoid(a2[1][r]);
                const float nn = tanhf(__fadd_rn(a3[2][r], __fmul_rn(rr, a1[0][r])));
                const float hn = __fadd_rn(__fmul_rn(__fsub_rn(1.0f, zz), nn), __fmul_rn(zz, h[r]));
                h[r] = hn;
                float mean, rstd;
                const float d = gmpe_wgrad::layer_norm_64(hn, p.eps, mean, rstd);
                if (ok) {
                    p.feat[m * H + lane] = __fadd_rn(__fmul_rn(__fmul_rn(d, rstd), lw), lb);
                    if (SAVE) {
                        float* g = p.sG + m * G4 + lane;
                        g[0] = rr; g[H] = zz; g[2 * H] = nn; g[3 * H] = a1[0][r];
                        p.sH[m * H + lane] = hn;
                        if (lane == 0) { p.sS[2 * m] = mean; p.sS[2 * m + 1] = rstd; }
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (row0 + r < p.Nb) p.hout[(row0 + r) * H + lane] = h[r];
    }
}

// backward 1: back-propagation through time of a tile (the head of this file)
__global__ __launch_bounds__(BLOCK) void k_gru_bptt(GruArgs p) {
    extern __shared__ __attribute__((aligned(16))) float sh[];
    float* w_ih = sh;                                   // [3H][64]
    float* w_hh = sh + G3 * H;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    float* dgw = sh + 2 * G3 * H + wv * R * G4;         // this wave's gate gradients [R][4][64]: dr, dz, dn, dhn
    double* cs = reinterpret_cast<double*>(sh + 2 * G3 * H + NW * R * G4);      // [NW][6H]
    for (int i = tid; i < G3 * H; i += BLOCK) { w_ih[i] = p.wih[i]; w_hh[i] = p.whh[i]; }
    const float lw = p.lnw[lane];
    __syncthreads();
    for (int64_t tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
        const int64_t row0 = tile * TILE + wv * R;
        double c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        float dh[R];
#pragma unroll
        for (int r = 0; r < R; ++r) dh[r] = (p.gho && row0 + r < p.Nb) ? p.gho[(row0 + r) * H + lane] : 0.0f;
        for (int64_t t = p.L - 1; t >= 0; --t) {
            float dtz[R], mk[R];                        // dh_t * z, added to the state gradient's chain at its end; the step's mask
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const bool ok = row0 + r < p.Nb;
                const int64_t m = t * p.Nb + row0 + r;
                float rr = 0.0f, zz = 0.0f, nn = 0.0f, hn = 0.0f, hc = 0.0f, mean = 0.0f, rstd = 0.0f, g = 0.0f, hp = 0.0f;
                mk[r] = 0.0f;
                if (ok) {
                    const float* s = p.sG + m * G4 + lane;
                    rr = s[0]; zz = s[H]; nn = s[2 * H]; hn = s[3 * H];
                    hc = p.sH[m * H + lane];
                    mean = p.sS[2 * m]; rstd = p.sS[2 * m + 1];
                    g = p.gf[m * H + lane];
                    mk[r] = p.masks[m];
                    hp = __fmul_rn(t > 0 ? p.sH[(m - p.Nb) * H + lane] : p.hxs[(row0 + r) * H + lane], mk[r]);
                }
                const float xh = __fmul_rn(__fsub_rn(hc, mean), rstd);
                const float dxh = __fmul_rn(g, lw);
                const float dln = gmpe_wgrad::layer_norm_64_backward(dxh, xh, rstd);
                const float dt = __fadd_rn(dh[r], dln);
                const float dz = __fmul_rn(dt, __fsub_rn(hp, nn)), dn = __fmul_rn(dt, __fsub_rn(1.0f, zz));
                dtz[r] = __fmul_rn(dt, zz);
                const float dnp = __fmul_rn(dn, __fsub_rn(1.0f, __fmul_rn(nn, nn)));
                const float dzp = __fmul_rn(__fmul_rn(dz, zz), __fsub_rn(1.0f, zz));
                const float dhn = __fmul_rn(dnp, rr);
                const float drp = __fmul_rn(__fmul_rn(__fmul_rn(dnp, hn), rr), __fsub_rn(1.0f, rr));
                float* dg = dgw + r * G4 + lane;
                dg[0] = drp; dg[H] = dzp; dg[2 * H] = dnp; dg[3 * H] = dhn;
                if (ok) {
                    float* o = p.dG + m * G4 + lane;
                    o[0] = drp; o[H] = dzp; o[2 * H] = dnp; o[3 * H] = dhn;
                    c[0] += (double)drp; c[1] += (double)dzp; c[2] += (double)dnp; c[3] += (double)dhn;
                    c[4] += (double)g * (double)xh; c[5] += (double)g;
                }
            }
            __syncthreads();
            float ax[R], ah[R];
#pragma unroll
            for (int r = 0; r < R; ++r) ax[r] = ah[r] = 0.0f;
#pragma unroll 1
            for (int gi = 0; gi < G3; gi += 4) {        // gate gi / 64, rows gi .. gi+3 of both matrices
                float wi[4], wh[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) { wi[i] = w_ih[(gi + i) * H + lane]; wh[i] = w_hh[(gi + i) * H + lane]; }
                const int hoff = gi >= 2 * H ? gi + H : gi;                     // the n gate of W_hh takes dhn
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const float4 a = *reinterpret_cast<const float4*>(dgw + r * G4 + gi);
                    const float4 b = *reinterpret_cast<const float4*>(dgw + r * G4 + hoff);
                    float u = ax[r], v = ah[r];
                    u = fmaf(wi[0], a.x, u); u = fmaf(wi[1], a.y, u); u = fmaf(wi[2], a.z, u); u = fmaf(wi[3], a.w, u);
                    v = fmaf(wh[0], b.x, v); v = fmaf(wh[1], b.y, v); v = fmaf(wh[2], b.z, v); v = fmaf(wh[3], b.w, v);
                    ax[r] = u; ah[r] = v;
                }
            }
            __syncthreads();                            // the next step overwrites dgw
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (row0 + r < p.Nb) p.gx[(t * p.Nb + row0 + r) * H + lane] = ax[r];
                dh[r] = __fmul_rn(__fadd_rn(dtz[r], ah[r]), mk[r]);        // the mask cuts the chain where forward zeroed h
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (row0 + r < p.Nb) p.ghxs[(row0 + r) * H + lane] = dh[r];
#pragma unroll
        for (int q = 0; q < 6; ++q) cs[wv * NCOL + q * H + lane] = c[q];
        __syncthreads();
        for (int i = tid; i < NCOL; i += BLOCK) {
            double s = cs[i];
            for (int w = 1; w < NW; ++w) s += cs[w * NCOL + i];
            p.partC[tile * NCOL + i] = s;
        }
        __syncthreads();
    }
}

// backward 2: part blockIdx.x of the rows, matrix blockIdx.y (0 .. 2: W_ih gates r, z, n; 3 .. 5: W_hh): out[j][d] = sum over the part's rows of
// dG[m][gate][j] * B[m][d], B = x or the masked previous state. Thread: j = tid / 4, d = 16 * (tid % 4) .. + 15.
__global__ __launch_bounds__(BLOCK) void k_gru_wgrad(GruArgs p) {
    const int y = blockIdx.y;
    const int col = y < 3 ? y * H : (y == 5 ? 3 * H : (y - 3) * H);             // column block of dG
    const int64_t m0 = (int64_t)blockIdx.x * p.part_rows, m1 = m0 + p.part_rows < p.M ? m0 + p.part_rows : p.M;
    gmpe_wgrad::part_products(
        m0, m1, [&](int64_t m, int k) { return p.dG[m * G4 + col + k]; },
        [&](int64_t m, int k) {
            if (y < 3) return p.x[m * H + k];
            return __fmul_rn(m >= p.Nb ? p.sH[(m - p.Nb) * H + k] : p.hxs[m * H + k], p.masks[m]);
        },
        p.partW + ((int64_t)blockIdx.x * 6 + y) * H * H);
}

// backward 3: the partial sums in their fixed order, rounded once. Workgroups 0 .. 95: one weight element per thread; 96 .. 119: 16 columns of partC each.
constexpr int FIN_W_BLOCKS = 2 * G3 * H / BLOCK, FIN_C_BLOCKS = NCOL / FIN_COLS;
__global__ __launch_bounds__(BLOCK) void k_gru_finish(GruArgs p) {
    __shared__ double cs[FIN_SLICES][FIN_COLS];
    const int tid = threadIdx.x;
    if (blockIdx.x < FIN_W_BLOCKS) {
        const int e = blockIdx.x * BLOCK + tid;         // (matrix 0 .. 5, j, d) as in partW
        const double s = gmpe_wgrad::sum_parts(p.partW, p.nparts, 2 * G3 * H, e);
        if (e < G3 * H) p.gwih[e] = (float)s; else p.gwhh[e - G3 * H] = (float)s;
        return;
    }
    const int col = ((int)blockIdx.x - FIN_W_BLOCKS) * FIN_COLS + tid % FIN_COLS;
    const double tot = gmpe_wgrad::sum_slices(p.partC, p.ntiles, NCOL, col - tid % FIN_COLS, cs);
    if (tid >= FIN_COLS) return;
    const float v = (float)tot;
    const int q = col / H, jj = col % H;
    if (q == 0 || q == 1) { p.gbih[q * H + jj] = v; p.gbhh[q * H + jj] = v; }
    else if (q == 2) p.gbih[2 * H + jj] = v;
    else if (q == 3) p.gbhh[2 * H + jj] = v;
    else if (q == 4) p.glnw[jj] = v;
    else p.glnb[jj] = v;
}

using gmpe::fail;

struct Layout { size_t sG, sH, sS, dG, partC, partW, total; int64_t ntiles; int nparts; int64_t part_rows; };

bool layout(int64_t L, int64_t Nb, Layout& y) {
    if (L < 1 || Nb < 1 || L > (int64_t)1 << 40 || Nb > ((int64_t)1 << 40) / L) return false;      // M * 4H * 4 bytes stays far inside int64
    const int64_t M = L * Nb;
    y.ntiles = (Nb + TILE - 1) / TILE;
    const gmpe_wgrad::Parts parts = gmpe_wgrad::partition(M);
    y.nparts = parts.nparts; y.part_rows = parts.part_rows;
    gmpe::Carver c;
    y.partC = c.take((size_t)y.ntiles * NCOL * sizeof(double));
    y.partW = c.take((size_t)y.nparts * 2 * G3 * H * sizeof(double));
    y.sG = c.take((size_t)M * G4 * sizeof(float));
    y.dG = c.take((size_t)M * G4 * sizeof(float));
    y.sH = c.take((size_t)M * H * sizeof(float));
    y.sS = c.take((size_t)M * 2 * sizeof(float));
    y.total = c.total();
    return true;
}

// the checks both entry points make alike, before any device call
int check_plan(const char* fn, const gmpe_gru_plan* pl, bool backward, Layout& y) {
    if (!pl) return fail(fn, "null plan");
    if (pl->steps < 1) return fail(fn, "steps must be >= 1");
    if (pl->rows < 1) return fail(fn, "rows must be >= 1");
    if (pl->in_dim != H || pl->hidden != H)
        return fail(fn, "unsupported (in_dim, hidden) = (" + std::to_string(pl->in_dim) + ", " + std::to_string(pl->hidden) + "): only (64, 64) is built");
    if (!(pl->eps > 0.0)) return fail(fn, "eps must be > 0");
    if (!layout(pl->steps, pl->rows, y)) return fail(fn, "steps * rows is too large");
    if (y.ntiles > 0x7fffffffLL) return fail(fn, "rows: too many for one launch");
    const gmpe::PtrField ptrs[] = {
        {pl->x, "x", true}, {pl->hxs, "hxs", true}, {pl->masks, "masks", true}, {pl->weight_ih, "weight_ih", true}, {pl->weight_hh, "weight_hh", true},
        {pl->bias_ih, "bias_ih", true}, {pl->bias_hh, "bias_hh", true}, {pl->ln_weight, "ln_weight", true}, {pl->ln_bias, "ln_bias", true},
        {pl->features, "features", !backward}, {pl->hxs_out, "hxs_out", !backward}, {pl->grad_features, "grad_features", backward},
        {pl->grad_hxs_out, "grad_hxs_out", false}, {pl->grad_x, "grad_x", backward}, {pl->grad_hxs, "grad_hxs", backward},
        {pl->grad_weight_ih, "grad_weight_ih", backward}, {pl->grad_weight_hh, "grad_weight_hh", backward}, {pl->grad_bias_ih, "grad_bias_ih", backward},
        {pl->grad_bias_hh, "grad_bias_hh", backward}, {pl->grad_ln_weight, "grad_ln_weight", backward}, {pl->grad_ln_bias, "grad_ln_bias", backward}};
    if (int rc = gmpe::check_ptrs(fn, ptrs)) return rc;
    if (int rc = gmpe::check_workspace(fn, pl->workspace, pl->workspace_bytes, y.total, backward, "workspace is required (the one gmpe_gru_forward filled)",
                                       "gmpe_gru_workspace_bytes(steps, rows, hidden, 1)"))
        return rc;
    if (!backward) {                                    // hxs_out against everything the launch reads or writes
        const size_t M = (size_t)pl->steps * (size_t)pl->rows, fb = sizeof(float);
        const uintptr_t a0 = (uintptr_t)pl->hxs_out, a1 = a0 + (size_t)pl->rows * H * fb;
        const struct { const void* ptr; size_t bytes; const char* name; } rng[] = {
            {pl->x, M * H * fb, "x"}, {pl->masks, M * fb, "masks"}, {pl->weight_ih, (size_t)G3 * H * fb, "weight_ih"}, {pl->weight_hh, (size_t)G3 * H * fb, "weight_hh"},
            {pl->bias_ih, G3 * fb, "bias_ih"}, {pl->bias_hh, G3 * fb, "bias_hh"}, {pl->ln_weight, H * fb, "ln_weight"}, {pl->ln_bias, H * fb, "ln_bias"},
            {pl->features, M * H * fb, "features"}, {pl->workspace, pl->workspace ? pl->workspace_bytes : 0, "workspace"},
            {pl->hxs, (size_t)pl->rows * H * fb, "hxs"}};
        for (const auto& q : rng) {
            const uintptr_t b0 = (uintptr_t)q.ptr, b1 = b0 + q.bytes;
            if (!q.bytes || a1 <= b0 || b1 <= a0) continue;
            if (q.ptr == pl->hxs && b0 == a0) {
                if (pl->workspace) return fail(fn, "hxs_out may be hxs in a forward-only plan only (backward reads hxs)");
                continue;
            }
            return fail(fn, std::string("hxs_out overlaps ") + q.name);
        }
    }
    return GMPE_OK;
}

GruArgs bind(const gmpe_gru_plan* pl, const Layout& y) {
    GruArgs a;
    a.L = pl->steps; a.Nb = pl->rows; a.M = pl->steps * pl->rows; a.ntiles = y.ntiles; a.part_rows = y.part_rows; a.nparts = y.nparts;
    a.eps = (float)pl->eps;
    a.x = pl->x; a.hxs = pl->hxs; a.masks = pl->masks; a.wih = pl->weight_ih; a.whh = pl->weight_hh; a.bih = pl->bias_ih; a.bhh = pl->bias_hh;
    a.lnw = pl->ln_weight; a.lnb = pl->ln_bias; a.feat = pl->features; a.hout = pl->hxs_out;
    void* w = pl->workspace;
    a.sG = gmpe::at<float>(w, y.sG); a.sH = gmpe::at<float>(w, y.sH); a.sS = gmpe::at<float>(w, y.sS);
    a.dG = gmpe::at<float>(w, y.dG); a.partC = gmpe::at<double>(w, y.partC); a.partW = gmpe::at<double>(w, y.partW);
    a.gf = pl->grad_features; a.gho = pl->grad_hxs_out; a.gx = pl->grad_x; a.ghxs = pl->grad_hxs; a.gwih = pl->grad_weight_ih; a.gwhh = pl->grad_weight_hh;
    a.gbih = pl->grad_bias_ih; a.gbhh = pl->grad_bias_hh; a.glnw = pl->grad_ln_weight; a.glnb = pl->grad_ln_bias;
    return a;
}

}  // namespace

extern "C" {

int gmpe_gru_workspace_bytes(int64_t steps, int64_t rows, int32_t hidden, int32_t want_backward, size_t* bytes_out) {
    const char* fn = "gmpe_gru_workspace_bytes";
    Layout y;
    const std::string dims = hidden != H ? "unsupported hidden = " + std::to_string(hidden) + ": only 64 is built" : std::string();
    if (int rc = gmpe::check_workspace_query(fn, bytes_out, dims, want_backward)) return rc;
    if (!layout(steps, rows, y)) return fail(fn, "steps and rows must be >= 1 (and their product not absurd)");
    *bytes_out = want_backward ? y.total : 0;
    return GMPE_OK;
}

int gmpe_gru_forward(int device, const gmpe_gru_plan* pl, void* stream) {
    Layout y;
    if (int rc = check_plan("gmpe_gru_forward", pl, false, y)) return rc;
    GMPE_HIP_CHECK(hipSetDevice(device));
    const bool save = pl->workspace != nullptr;
    void (*fn)(GruArgs) = save ? k_gru_fwd<true> : k_gru_fwd<false>;
    if (int rc = gmpe::raise_dynamic_lds_once(reinterpret_cast<const void*>(fn), device, save ? 1 : 0, FWD_LDS)) return rc;
    const GruArgs a = bind(pl, y);
    GMPE_LAUNCH(fn, dim3((unsigned)gmpe::resident_grid(y.ntiles, FWD_LDS, 1)), dim3(BLOCK), FWD_LDS, static_cast<hipStream_t>(stream), a);
    return GMPE_OK;
}

int gmpe_gru_backward(int device, const gmpe_gru_plan* pl, void* stream) {
    Layout y;
    if (int rc = check_plan("gmpe_gru_backward", pl, true, y)) return rc;
    GMPE_HIP_CHECK(hipSetDevice(device));
    if (int rc = gmpe::raise_dynamic_lds_once(reinterpret_cast<const void*>(k_gru_bptt), device, 2, BPTT_LDS)) return rc;
    const GruArgs a = bind(pl, y);
    hipStream_t st = static_cast<hipStream_t>(stream);
    GMPE_LAUNCH(k_gru_bptt, dim3((unsigned)gmpe::resident_grid(y.ntiles, BPTT_LDS, 1)), dim3(BLOCK), BPTT_LDS, st, a);
    GMPE_LAUNCH(k_gru_wgrad, dim3((unsigned)y.nparts, 6), dim3(BLOCK), 0, st, a);
    GMPE_LAUNCH(k_gru_finish, dim3(FIN_W_BLOCKS + FIN_C_BLOCKS), dim3(BLOCK), 0, st, a);
    return GMPE_OK;
}

}  // extern "C"
