// gmpe_ppo_popart.hip — the loss arithmetic of one PPO minibatch when the value normaliser is the critic's output layer v_out = PopArt(H, 1)
// (include/gmpe.h gmpe_ppo_loss_popart). The critic hands over its FEATURES; the kernels evaluate v_out, update its statistics, compute the losses of
// gmpe_ppo_loss.hip, leave the gradients with respect to features, weight and bias, and rescale the layer, in the reference's order:
//   * values = F.linear(features, W, b) inside evaluate_actions, BEFORE the update (graph_mappo.py:160-172, graph_actor_critic.py:395, popart.py:55-60);
//   * cal_value_loss: PopArt.update(returns) then normalize(returns) (graph_mappo.py:92-97, popart.py:62-99);
//   * the policy block, the value branch and the means exactly as gmpe_ppo_loss.hip (the row code is gmpe_ppo_rows.h, shared).
// PopArt.update, float32, over all rows (no mask), restated with its quirks:
//   mean.mul_(beta).add_(batch_mean * (1 - beta)), the same for mean_sq, debiasing_term.mul_(beta).add_(1 - beta)            in place
//   stddev' = clamp(sqrt(mean_sq - mean^2), 1e-4)        the RAW statistics, not the debiased ones; NaN stays NaN (torch.clamp keeps it)
//   W'      = (W * stddev) / stddev'
//   b'      = ((stddev * b + mean') - mean') / stddev'   old_mean is an alias of self.mean, so it is already the NEW mean when it is read
// normalize: mean_d = mean / clamp(debiasing_term, eps), sd = sqrt(clamp(mean_sq / clamp(...) - mean_d^2, 1e-2)), R = (returns - mean_d) / sd.
//
// Launches: stats (double sums of returns, returns^2, active_masks) -> prepare (the update into the workspace header; mean, mean_sq, debiasing_term in
// place) -> rows -> finish (scalars, grad_weight, grad_bias, then W', b', stddev' — published last, so they may overwrite W, b, stddev).
//
// The row pass. A workgroup owns TILE = 256 rows; wave w owns rows 64w .. 64w+63 of the tile in both of its mappings:
//   feature mapping: the H columns are cut in quads (4q .. 4q+3; the last may be short), NQ = ceil(H / 4), L = the power of two >= NQ (at most 64).
//     A wave works on 64 / L rows at once: lane = sub * L + c reads quads c, c + L, c + 2L, ... (at most 4: H <= 1024) of row (pass * 64 / L + sub),
//     so with H = 64 a wave instruction moves four whole rows, 1 KiB contiguous, 16 bytes per lane. Nothing of this goes through LDS.
//   dot product (the fixed order, a function of H alone): a lane adds its products in column order from 0.0f, the L lanes are added by an xor tree
//     (offsets 1, 2, .. L/2; the lower lane is the left operand), then + b. The value goes to the row's own lane through 1 KiB of LDS.
//   row mapping: lane i of the workgroup is row i, as in gmpe_ppo_loss.hip: policy block, value branch, g = d value_loss / d v.
//   back in the feature mapping: grad_features = g * W_j (one float32 product) and the double sums of g * F_rj, per lane over its passes, then across the
//     64 / L row groups of the wave (xor tree), then across the four waves in wave order: one [H] partial per workgroup, merged by `finish` in a fixed
//     order. The features are read a second time here: the tile (64 KiB at H = 64) was read by this workgroup microseconds before and comes from L2.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include <atomic>
#include <string>

#include "../../include/gmpe.h"
#include "gmpe_ppo_rows.h"

#pragma clang fp contract(off)

namespace gmpe {
int report_error(int code, const std::string& m);   // gmpe_step.hip: the library's gmpe_last_error text
}

namespace {

using namespace gmpe_ppo;

constexpr int NROWP = 5;          // sum -min(surr1, surr2) * w, sum H * w, sum value_loss * w, sum ratio, sum g (d value_loss / d bias)
constexpr int HDR_DOUBLES = 8;    // D_policy, D_value, then f32: mean_d, sd, stddev, stddev', b' (three doubles), the rest spare
constexpr int MAXQ = GMPE_POPART_MAX_HIDDEN / 4 / 64;   // quads per lane and row at the largest H
constexpr int FIN_COLS = 16, FIN_SLICES = TILE / FIN_COLS;   // finish: 16 columns per workgroup, 16 slices of the partials per column
static_assert(MAXQ == 4, "the feature mapping holds at most four quads per lane");

struct PopArgs {
    int64_t B;
    int K, S, flags;               // as LossArgs of gmpe_ppo_loss.hip
    uint32_t magic;
    int H, NQ, L, lsh, vecf;       // NQ = ceil(H / 4); L = 1 << lsh lanes per row; vecf: features and grad_features move in 16-byte units
    const float *logits, *avail, *feat, *W, *bias, *stddev, *old_lp, *adv, *vp, *ret, *am;
    const void* actions;
    float *grad_logits, *grad_feat, *grad_W, *grad_b, *values_out, *out_lp, *out_ratio, *W_out, *bias_out, *stddev_out;
    float lo, hi, clip, delta, half_delta, ent_coef, wbeta, w1beta, eps;
    float *mean, *mean_sq, *db;
    double *stat_part, *row_part, *col_part, *hdr, *out;
};

// torch.clamp(x, min=lo): NaN stays NaN (fmaxf would return lo)
__device__ __forceinline__ float clamp_min(float x, float lo) { return x != x ? x : fmaxf(x, lo); }

// 1: per-workgroup double sums of returns, returns^2, active_masks
__global__ __launch_bounds__(TILE) void k_pop_stats(PopArgs p) {
    __shared__ double red[NW * NSTAT];
    stats_tile(p.ret, p.am, p.B, p.stat_part, red);
}

// 2: merge; PopArt.update (popart.py:62-83) BEFORE normalize, as cal_value_loss does. The new weight is left to `finish`; stddev' and b' wait in the header.
__global__ __launch_bounds__(TILE) void k_pop_prepare(PopArgs p, int64_t nparts) {
    __shared__ double sh[TILE][NSTAT];
    merge<NSTAT>(p.stat_part, nparts, sh);
    if (threadIdx.x != 0) return;
    const double n = (double)p.B, msum = sh[0][2];
    p.hdr[0] = (p.flags & GMPE_PPO_POLICY_ACTIVE_MASKS) ? msum : n;
    p.hdr[1] = (p.flags & GMPE_PPO_VALUE_ACTIVE_MASKS) ? msum : n;
    const float bm = (float)(sh[0][0] / n), bsq = (float)(sh[0][1] / n);                     // input_vector.mean(0), (input_vector ** 2).mean(0)
    const float s_old = *p.stddev, b = *p.bias;                                              // old_stddev; old_mean is NOT kept: it aliases self.mean
    const float mean = __fadd_rn(__fmul_rn(*p.mean, p.wbeta), __fmul_rn(bm, p.w1beta));      // mean.mul_(beta).add_(batch_mean * (1.0 - beta))
    const float msq = __fadd_rn(__fmul_rn(*p.mean_sq, p.wbeta), __fmul_rn(bsq, p.w1beta));
    const float db = __fadd_rn(__fmul_rn(*p.db, p.wbeta), p.w1beta);                         // debiasing_term.mul_(beta).add_(1.0 * (1.0 - beta))
    *p.mean = mean; *p.mean_sq = msq; *p.db = db;
    const float s_new = clamp_min(__fsqrt_rn(__fsub_rn(msq, __fmul_rn(mean, mean))), 1e-4f);         // (mean_sq - mean ** 2).sqrt().clamp(min=1e-4)
    const float b_new = __fdiv_rn(__fsub_rn(__fadd_rn(__fmul_rn(s_old, b), mean), mean), s_new);     // (old_stddev * bias + old_mean - mean) / stddev
    const float dc = clamp_min(db, p.eps);                                                           // debiased_mean_var (popart.py:85-89)
    const float mean_d = __fdiv_rn(mean, dc);
    const float var = clamp_min(__fsub_rn(__fdiv_rn(msq, dc), __fmul_rn(mean_d, mean_d)), 1e-2f);
    float* f = reinterpret_cast<float*>(p.hdr + 2);
    f[0] = mean_d; f[1] = __fsqrt_rn(var); f[2] = s_old; f[3] = s_new; f[4] = b_new;
}

// one quad of a features row: columns 4q .. 4q+3 (those below H)
__device__ __forceinline__ void load_quad(const float* __restrict__ fr, int q, int H, bool vec, float (&f)[4]) {
    if (vec) {
        const float4 t = *reinterpret_cast<const float4*>(fr + 4 * q);
        f[0] = t.x; f[1] = t.y; f[2] = t.z; f[3] = t.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = 4 * q + i < H ? fr[4 * q + i] : 0.0f;
    }
}

// 3: the row pass (the head of this file)
template <bool VEC, bool ACT64>
__global__ __launch_bounds__(TILE) void k_pop_rows(PopArgs p) {
    extern __shared__ __attribute__((aligned(16))) float sh[];              // the logits tile [TILE, S], then the column sums: 4 * L * MAXQ doubles
    __shared__ double red[NW * NROWP];
    __shared__ float vsh[TILE], gsh[TILE];                                  // a row's value / gradient between the two mappings
    const int K = p.K, S = p.S, H = p.H, NQ = p.NQ, L = p.L;
    const int64_t row0 = (int64_t)blockIdx.x * TILE, r = row0 + threadIdx.x;
    const int rows = p.B - row0 < TILE ? (int)(p.B - row0) : TILE, n = rows * K;
    const bool live = (int)threadIdx.x < rows;
    float* row = sh + threadIdx.x * S;
    double* colsum = reinterpret_cast<double*>(sh + ((TILE * S + 3) & ~3));
    const int64_t g0 = row0 * K;
    const bool vecf = p.vecf;

    // ---- feature mapping: the value of every row of the tile
    const int lane = threadIdx.x & 63, wv0 = (int)(threadIdx.x >> 6) * 64;
    const int c = lane & (L - 1), sub = lane >> p.lsh, RP = 64 >> p.lsh;    // RP rows per pass, L passes
    float wq[MAXQ][4];
#pragma unroll
    for (int k = 0; k < MAXQ; ++k)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int col = 4 * (c + k * L) + i;
            wq[k][i] = col < H ? p.W[col] : 0.0f;
        }
    const float bias = *p.bias;
    for (int ps = 0; ps < L; ++ps) {
        const int lr = wv0 + ps * RP + sub;
        float acc = 0.0f;
        if (lr < rows) {
            const float* fr = p.feat + (row0 + lr) * H;
#pragma unroll
            for (int k = 0; k < MAXQ; ++k) {
                const int q = c + k * L;
                if (q < NQ) {
                    float f[4];
                    load_quad(fr, q, H, vecf, f);
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (4 * q + i < H) acc = __fadd_rn(acc, __fmul_rn(f[i], wq[k][i]));
                }
            }
        }
        for (int off = 1; off < L; off <<= 1) {                             // every lane of the wave takes part; lanes of other rows are never mixed in
            const float o = __shfl_xor(acc, off);
            acc = (lane & off) ? __fadd_rn(o, acc) : __fadd_rn(acc, o);
        }
        if (c == 0 && lr < rows) vsh[lr] = __fadd_rn(acc, bias);
    }

    // ---- row mapping: the policy block and the value branch, as gmpe_ppo_loss.hip
    uint64_t avail = ~0ull;
    if (p.avail) {
        tile_copy<VEC, true>(const_cast<float*>(p.avail) + g0, sh, n, K, S, p.magic);
        __syncthreads();
        if (live) avail = avail_bits(row, K);
        __syncthreads();
    }
    tile_copy<VEC, true>(const_cast<float*>(p.logits) + g0, sh, n, K, S, p.magic);
    __syncthreads();                                                        // also orders vsh

    double acc[NROWP] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (live) {
        const double Dp = p.hdr[0], Dv = p.hdr[1];
        const float am = p.am[r];
        const float wp = (p.flags & GMPE_PPO_POLICY_ACTIVE_MASKS) ? am : 1.0f, wv = (p.flags & GMPE_PPO_VALUE_ACTIVE_MASKS) ? am : 1.0f;
        PolicyRow q;
        q.avail = avail;
        q.action = ACT64 ? static_cast<const int64_t*>(p.actions)[r] : (int64_t)static_cast<const float*>(p.actions)[r];
        q.adv = p.adv[r]; q.old_lp = p.old_lp[r]; q.wp = wp; q.Dp = (float)Dp; q.lo = p.lo; q.hi = p.hi; q.ent_coef = p.ent_coef;
        float la, ratio;
        policy_row(row, K, q, &la, &ratio, &acc[0], &acc[1]);
        acc[3] = (double)ratio;
        if (p.out_lp) p.out_lp[r] = la;
        if (p.out_ratio) p.out_ratio[r] = ratio;
        const float v = vsh[threadIdx.x];
        if (p.values_out) p.values_out[r] = v;
        const float* st = reinterpret_cast<const float*>(p.hdr + 2);
        const float R = __fdiv_rn(__fsub_rn(p.ret[r], st[0]), st[1]);       // normalize: (returns - mean_d) / sqrt(var_d)
        const float g = value_row<true>(v, p.vp[r], R, p.flags & GMPE_PPO_HUBER_LOSS, p.flags & GMPE_PPO_CLIPPED_VALUE_LOSS, p.clip, p.delta, p.half_delta, wv,
                                  (float)Dv, &acc[2]);
        gsh[threadIdx.x] = g;
        acc[4] = (double)g;
    }
    block_sum<NROWP>(acc, red, p.row_part + (int64_t)blockIdx.x * NROWP);    // its barrier also orders gsh and the gradient rows before the copy out
    tile_copy<VEC, false>(p.grad_logits + g0, sh, n, K, S, p.magic);

    // ---- feature mapping again: grad_features, and this workgroup's double sums of g * F over its rows
    double da[MAXQ][4];
#pragma unroll
    for (int k = 0; k < MAXQ; ++k)
#pragma unroll
        for (int i = 0; i < 4; ++i) da[k][i] = 0.0;
    for (int ps = 0; ps < L; ++ps) {
        const int lr = wv0 + ps * RP + sub;
        if (lr < rows) {
            const float g = gsh[lr];
            const double gd = (double)g;
            const float* fr = p.feat + (row0 + lr) * H;
            float* gr = p.grad_feat + (row0 + lr) * H;
#pragma unroll
            for (int k = 0; k < MAXQ; ++k) {
                const int q = c + k * L;
                if (q < NQ) {
                    float f[4];
                    load_quad(fr, q, H, vecf, f);
#pragma unroll
                    for (int i = 0; i < 4; ++i) da[k][i] += gd * (double)f[i];           // the product is exact in double
                    if (vecf) {
                        *reinterpret_cast<float4*>(gr + 4 * q) = make_float4(__fmul_rn(g, wq[k][0]), __fmul_rn(g, wq[k][1]), __fmul_rn(g, wq[k][2]),
                                                                             __fmul_rn(g, wq[k][3]));
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (4 * q + i < H) gr[4 * q + i] = __fmul_rn(g, wq[k][i]);
                    }
                }
            }
        }
    }
    for (int off = L; off < 64; off <<= 1)                                  // the wave's 64 / L row groups, the lower lane the left operand
#pragma unroll
        for (int k = 0; k < MAXQ; ++k)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const double o = __shfl_xor(da[k][i], off);
                da[k][i] = (lane & off) ? o + da[k][i] : da[k][i] + o;
            }
    for (int w = 0; w < NW; ++w) {                                          // the four waves in wave order, through colsum[4 * L * MAXQ]
        if (wv0 == w * 64 && sub == 0)
#pragma unroll
            for (int k = 0; k < MAXQ; ++k)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int col = 4 * (c + k * L) + i;
                    colsum[col] = w == 0 ? da[k][i] : colsum[col] + da[k][i];
                }
        __syncthreads();
    }
    for (int j = threadIdx.x; j < H; j += TILE) p.col_part[(int64_t)blockIdx.x * H + j] = colsum[j];
}

// 4: the partials -> the scalar row, grad_bias and b', stddev' (workgroup 0); grad_weight and W' (the others, FIN_COLS columns each)
__global__ __launch_bounds__(TILE) void k_pop_finish(PopArgs p, int64_t nparts) {
    __shared__ double sh[TILE][NROWP];
    const float* st = reinterpret_cast<const float*>(p.hdr + 2);
    if (blockIdx.x == 0) {
        merge<NROWP>(p.row_part, nparts, sh);
        if (threadIdx.x != 0) return;
        const double Dp = p.hdr[0], Dv = p.hdr[1];
        const double pol = sh[0][0] / Dp, ent = sh[0][1] / Dp;
        p.out[GMPE_PPO_OUT_POLICY_LOSS] = pol;
        p.out[GMPE_PPO_OUT_DIST_ENTROPY] = ent;
        p.out[GMPE_PPO_OUT_ACTOR_LOSS] = pol - (double)p.ent_coef * ent;
        p.out[GMPE_PPO_OUT_VALUE_LOSS] = sh[0][2] / Dv;
        p.out[GMPE_PPO_OUT_RATIO_MEAN] = sh[0][3] / (double)p.B;
        p.out[GMPE_PPO_OUT_DENOM_POLICY] = Dp;
        p.out[GMPE_PPO_OUT_DENOM_VALUE] = Dv;
        *p.grad_b = (float)sh[0][4];
        *p.stddev_out = st[3];                                              // every reader of stddev, bias and weight has finished: the row pass is over
        *p.bias_out = st[4];                                                // and this launch takes them from the header
        return;
    }
    // column j of col_part [nparts, H]: slice s adds partials s, s + FIN_SLICES, ... in order, the slices are added in slice order
    double (*cs)[FIN_COLS] = reinterpret_cast<double (*)[FIN_COLS]>(&sh[0][0]);
    static_assert(sizeof(sh) >= sizeof(double) * FIN_SLICES * FIN_COLS, "the slice sums fit the scalar block's LDS");
    const int jc = threadIdx.x % FIN_COLS, s = threadIdx.x / FIN_COLS, j = ((int)blockIdx.x - 1) * FIN_COLS + jc;
    double sum = 0.0;
    if (j < p.H)
        for (int64_t i = s; i < nparts; i += FIN_SLICES) sum += p.col_part[i * p.H + j];
    cs[s][jc] = sum;
    __syncthreads();
    if (s == 0 && j < p.H) {
        double tot = cs[0][jc];
        for (int q = 1; q < FIN_SLICES; ++q) tot += cs[q][jc];
        p.grad_W[j] = (float)tot;
        p.W_out[j] = __fdiv_rn(__fmul_rn(p.W[j], st[2]), st[3]);            // (weight * old_stddev) / stddev; W_out may be W: same thread, read first
    }
}

int64_t num_tiles(int64_t rows) { return (rows + TILE - 1) / TILE; }

int fail(int code, const std::string& m) { return gmpe::report_error(code, m); }

}  // namespace

#define LCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(GMPE_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

extern "C" {

int gmpe_ppo_loss_popart_workspace_bytes(int64_t rows, int32_t hidden, size_t* bytes_out) {
    if (!bytes_out || rows < 1 || hidden < 1 || hidden > GMPE_POPART_MAX_HIDDEN)
        return fail(GMPE_ERR_INVALID_ARG, "gmpe_ppo_loss_popart_workspace_bytes: bad arguments");
    *bytes_out = ((size_t)num_tiles(rows) * (NSTAT + NROWP + (size_t)hidden) + HDR_DOUBLES) * sizeof(double);
    return GMPE_OK;
}

int gmpe_ppo_loss_popart(int device, const gmpe_popart_loss_plan* pl, void* stream) {
    if (!pl) return fail(GMPE_ERR_INVALID_ARG, "gmpe_ppo_loss_popart: null plan");
    const int known = GMPE_PPO_POLICY_ACTIVE_MASKS | GMPE_PPO_VALUE_ACTIVE_MASKS | GMPE_PPO_CLIPPED_VALUE_LOSS | GMPE_PPO_HUBER_LOSS;
    if (pl->flags & ~known) return fail(GMPE_ERR_INVALID_ARG, "gmpe_ppo_loss_popart: unknown flags (GMPE_PPO_VALUENORM is not accepted: PopArt is the normaliser)");
    if (pl->rows < 1) return fail(GMPE_ERR_INVALID_ARG, "gmpe_ppo_loss_popart: need rows >= 1");
    if (pl->n_actions < 1 || pl->n_actions > GMPE_PPO_MAX_ACTIONS)
        return fail(GMPE_ERR_INVALID_ARG, "gmpe_ppo_loss_popart: n_actions must be in 1 .. " + std::to_string(GMPE_PPO_MAX_ACTIONS));
    if (pl->hidden < 1 || pl->hidden > GMPE_POPART_MAX_HIDDEN)
        return fail(GMPE_ERR_INVALID_ARG, "gmpe_ppo_loss_popart: hidden must be in 1 .. " + std::to_string(GMPE_POPART_MAX_HIDDEN));
    if (pl->actions_int64 != 0 && pl->actions_int64 != 1) return fail(GMPE_ERR_INVALID_ARG, "gmpe_ppo_loss_popart: actions_int64 must be 0 or 1");
    if (!pl->logits || !pl->critic_features || !pl->actions || !pl->old_action_log_probs || !pl->adv_targ || !pl->value_preds || !pl->returns ||
        !pl->active_masks)
        return fail(GMPE_ERR_INVALID_ARG, "gmpe_ppo_loss_popart: logits, critic_features, actions, old_action_log_probs, adv_targ, value_preds, returns and "
                                          "active_masks are required");
    if (!pl->weight || !pl->bias || !pl->stddev || !pl->mean || !pl->mean_sq || !pl->debiasing_term || !pl->weight_out || !pl->bias_out || !pl->stddev_out)
        return fail(GMPE_ERR_INVALID_ARG, "gmpe_ppo_loss_popart: weight, bias, stddev, mean, mean_sq, debiasing_term, weight_out, bias_out and stddev_out are required");
    if (!pl->out || !pl->grad_logits || !pl->grad_features || !pl->grad_weight || !pl->grad_bias)
        return fail(GMPE_ERR_INVALID_ARG, "gmpe_ppo_loss_popart: out, grad_logits, grad_features, grad_weight and grad_bias are required");
    if (!(pl->clip_param >= 0.0) || !(pl->huber_delta >= 0.0) || !(pl->beta >= 0.0 && pl->beta <= 1.0) || !(pl->epsilon > 0.0) || pl->entropy_coef != pl->entropy_coef)
        return fail(GMPE_ERR_INVALID_ARG, "gmpe_ppo_loss_popart: need clip_param >= 0, huber_delta >= 0, 0 <= beta <= 1, epsilon > 0 and a number for entropy_coef");
    const uintptr_t a4 = (uintptr_t)pl->logits | (uintptr_t)pl->critic_features | (uintptr_t)pl->available_actions | (uintptr_t)pl->old_action_log_probs |
                         (uintptr_t)pl->adv_targ | (uintptr_t)pl->value_preds | (uintptr_t)pl->returns | (uintptr_t)pl->active_masks | (uintptr_t)pl->weight |
                         (uintptr_t)pl->bias | (uintptr_t)pl->stddev | (uintptr_t)pl->mean | (uintptr_t)pl->mean_sq | (uintptr_t)pl->debiasing_term |
                         (uintptr_t)pl->weight_out | (uintptr_t)pl->bias_out | (uintptr_t)pl->stddev_out | (uintptr_t)pl->values_out | (uintptr_t)pl->grad_logits |
                         (uintptr_t)pl->grad_features | (uintptr_t)pl->grad_weight | (uintptr_t)pl->grad_bias | (uintptr_t)pl->action_log_probs |
                         (uintptr_t)pl->imp_weights;
    if ((a4 & 3) || ((uintptr_t)pl->actions & (pl->actions_int64 ? 7 : 3)) || ((uintptr_t)pl->out & 7))
        return fail(GMPE_ERR_INVALID_ARG, "gmpe_ppo_loss_popart: f32 arrays must be 4-byte aligned, int64 actions and out 8-byte aligned");
    size_t need = 0;
    gmpe_ppo_loss_popart_workspace_bytes(pl->rows, pl->hidden, &need);
    if (!pl->workspace || pl->workspace_bytes < need || ((uintptr_t)pl->workspace & 7))
        return fail(GMPE_ERR_INVALID_ARG, "gmpe_ppo_loss_popart: needs an 8-byte aligned workspace of gmpe_ppo_loss_popart_workspace_bytes(rows, hidden)");
    const int64_t nt = num_tiles(pl->rows);
    if (nt > 0x7fffffffLL) return fail(GMPE_ERR_INVALID_ARG, "gmpe_ppo_loss_popart: too many rows for one launch");
    LCHK(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    PopArgs a;
    a.B = pl->rows; a.K = pl->n_actions; a.S = pl->n_actions | 1; a.flags = pl->flags;
    a.magic = (uint32_t)(0x100000000ULL / (uint64_t)(pl->n_actions > 1 ? pl->n_actions : 2)) + 1u;
    a.H = pl->hidden; a.NQ = (pl->hidden + 3) / 4;
    a.lsh = 0;
    while ((1 << a.lsh) < a.NQ && a.lsh < 6) ++a.lsh;
    a.L = 1 << a.lsh;
    a.vecf = pl->hidden % 4 == 0 && !(((uintptr_t)pl->critic_features | (uintptr_t)pl->grad_features) & 15);
    a.logits = pl->logits; a.avail = pl->available_actions; a.feat = pl->critic_features; a.W = pl->weight; a.bias = pl->bias; a.stddev = pl->stddev;
    a.old_lp = pl->old_action_log_probs; a.adv = pl->adv_targ; a.vp = pl->value_preds; a.ret = pl->returns; a.am = pl->active_masks; a.actions = pl->actions;
    a.grad_logits = pl->grad_logits; a.grad_feat = pl->grad_features; a.grad_W = pl->grad_weight; a.grad_b = pl->grad_bias; a.values_out = pl->values_out;
    a.out_lp = pl->action_log_probs; a.out_ratio = pl->imp_weights; a.W_out = pl->weight_out; a.bias_out = pl->bias_out; a.stddev_out = pl->stddev_out;
    // a Python float meets a float32 tensor as float32(value): 1.0 - clip_param, 1.0 - beta and huber_delta / 2 are formed in double first
    a.lo = (float)(1.0 - pl->clip_param); a.hi = (float)(1.0 + pl->clip_param); a.clip = (float)pl->clip_param;
    a.delta = (float)pl->huber_delta; a.half_delta = (float)(pl->huber_delta / 2.0); a.ent_coef = (float)pl->entropy_coef;
    a.wbeta = (float)pl->beta; a.w1beta = (float)(1.0 - pl->beta); a.eps = (float)pl->epsilon;
    a.mean = pl->mean; a.mean_sq = pl->mean_sq; a.db = pl->debiasing_term;
    a.stat_part = static_cast<double*>(pl->workspace);
    a.row_part = a.stat_part + nt * NSTAT;
    a.hdr = a.row_part + nt * NROWP;
    a.col_part = a.hdr + HDR_DOUBLES;
    a.out = pl->out;
    const dim3 grid((unsigned)nt), block(TILE), one(1);
    hipLaunchKernelGGL(k_pop_stats, grid, block, 0, st, a);
    LCHK(hipGetLastError());
    hipLaunchKernelGGL(k_pop_prepare, one, block, 0, st, a, nt);
    LCHK(hipGetLastError());
    const bool vec = !(((uintptr_t)pl->logits | (uintptr_t)pl->available_actions | (uintptr_t)pl->grad_logits) & 15);   // tiles start at multiples of 1 KiB
    const size_t lds = (size_t)((TILE * a.S + 3) & ~3) * sizeof(float) + (size_t)4 * a.L * MAXQ * sizeof(double);
    void (*fn)(PopArgs) = vec ? (pl->actions_int64 ? k_pop_rows<true, true> : k_pop_rows<true, false>)
                              : (pl->actions_int64 ? k_pop_rows<false, true> : k_pop_rows<false, false>);
    if (lds > 48 * 1024) {                                                    // large K or H; once per device and instantiation, at the largest size there is
        static std::atomic<bool> raised[64][4];
        const int v = (vec ? 2 : 0) | (pl->actions_int64 ? 1 : 0);
        if (device < 0 || device >= 64 || !raised[device][v].load()) {
            LCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)(((TILE * (GMPE_PPO_MAX_ACTIONS | 1) + 3) & ~3) * sizeof(float) + 4 * 64 * MAXQ * sizeof(double))));
            if (device >= 0 && device < 64) raised[device][v].store(true);
        }
    }
    hipLaunchKernelGGL(fn, grid, block, lds, st, a);
    LCHK(hipGetLastError());
    const dim3 fin(1 + (unsigned)((pl->hidden + FIN_COLS - 1) / FIN_COLS));
    hipLaunchKernelGGL(k_pop_finish, fin, block, 0, st, a, nt);
    LCHK(hipGetLastError());
    return GMPE_OK;
}

}  // extern "C"
