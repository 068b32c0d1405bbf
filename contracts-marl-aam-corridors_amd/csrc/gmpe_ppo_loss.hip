// gmpe_ppo_loss.hip — the loss arithmetic of one PPO minibatch between the policy head's logits / the critic's values and the two scalars
// GR_MAPPO.ppo_update calls .backward() on (include/gmpe.h gmpe_ppo_loss). Handle-less, like gmpe_compute_returns.
//
// What is restated (the reference runs it as ~30 torch ops forward and as many backward):
//   * Categorical.forward + FixedCategorical.log_probs / entropy through ACTLayer.evaluate_actions (onpolicy/algorithms/utils/distributions.py:84-91,
//     act.py:212-220): x = logits with finfo(float32).min where available_actions == 0; l = x - logsumexp(x); p = softmax(l);
//     log-prob l[a]; entropy -sum p * clamp(l, finfo.min);
//   * the ratio / clip / surrogate block (onpolicy/algorithms/graph_mappo.py:176-197);
//   * cal_value_loss with ValueNorm.update then normalize (graph_mappo.py:89-117, onpolicy/utils/valuenorm.py:48-85) and huber_loss / mse_loss
//     (onpolicy/utils/util.py:24-30).
// Per-row arithmetic is float32 in the reference's operation order where one exists (no contraction); sums over rows are double, per-workgroup
// partials merged in a fixed order: no atomics, the same bits for the same rows wherever they lie in memory.
//
// Gradients, in closed form (row r, column j, a = the action, D = the denominator of the mean: sum of active_masks or B):
//   policy head   dlogp/dz_j = [j == a] - p_j;   dH/dz_j = -p_j * (l_j + H);   both 0 at masked entries: distributions.py:89 overwrites those logits
//                 in place, so no gradient reaches them.
//                 d min(surr1, surr2)/d ratio = adv where surr1 < surr2, or surr1 == surr2 with 1 - clip <= ratio <= 1 + clip (torch.min splits a tie in
//                 halves and clamp passes gradient on its closed range: half + half inside, half of adv = 0 outside, where a tie needs adv == 0); else 0.
//                 d actor_loss/dz_j = -(w/D) * that * ratio * ([j == a] - p_j) + entropy_coef * (w/D) * p_j * (l_j + H)       (graph_mappo.py:176-207)
//   value branch  huber (util.py:24-27): a = |e| <= d, b = e > d (NOT |e| > d: loss and gradient are zero for e < -d), d/de = a * e + b * d;  mse: e.
//                 original branch d/dv = -f'(R - v); clipped branch d/dv = -f'(R - vp - clamp(v - vp, +-clip)) while -clip <= v - vp <= clip, else 0;
//                 torch.max takes the larger branch's gradient and the mean of the two at an exact tie.                      (graph_mappo.py:89-117)
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

using namespace gmpe_ppo;         // gmpe_ppo_rows.h: TILE, the fixed-order sums, tile_copy and the row arithmetic, shared with gmpe_ppo_popart.hip

constexpr int NROW = 4;           // sum -min(surr1, surr2) * w, sum H * w, sum value_loss * w, sum ratio
constexpr int HDR_DOUBLES = 4;    // D_policy, D_value, then f32 mean, std (one double), one spare

struct LossArgs {
    int64_t B;
    int K, S, flags;               // S: LDS row stride in dwords, odd, so the 32 lanes of a ds_read_b32 group (stride S) hit 32 distinct banks
    uint32_t magic;                // floor(2^32 / K) + 1: f / K == umulhi(f, magic) for f < 2^16 (a tile holds at most TILE * 64 floats)
    const float *logits, *avail, *values, *old_lp, *adv, *vp, *ret, *am;
    const void* actions;
    float *grad_logits, *grad_values, *out_lp, *out_ratio;
    float lo, hi, clip, delta, half_delta, ent_coef, wbeta, w1beta, eps;
    float *rm, *rms, *db;
    double *stat_part, *row_part, *hdr, *out;
};

// 1: per-workgroup double sums of returns, returns^2, active_masks
__global__ __launch_bounds__(TILE) void k_loss_stats(LossArgs p) {
    __shared__ double red[NW * NSTAT];
    stats_tile(p.ret, p.am, p.B, p.stat_part, red);
}

// 2: merge; ValueNorm.update (valuenorm.py:56-73), BEFORE the normalisation as cal_value_loss does (graph_mappo.py:93-97); running_mean_var (:48-54)
__global__ __launch_bounds__(TILE) void k_loss_prepare(LossArgs p, int64_t nparts) {
    __shared__ double sh[TILE][NSTAT];
    merge<NSTAT>(p.stat_part, nparts, sh);
    if (threadIdx.x != 0) return;
    const double n = (double)p.B, msum = sh[0][2];
    p.hdr[0] = (p.flags & GMPE_PPO_POLICY_ACTIVE_MASKS) ? msum : n;
    p.hdr[1] = (p.flags & GMPE_PPO_VALUE_ACTIVE_MASKS) ? msum : n;
    float mean = 0.0f, sd = 1.0f;
    if (p.flags & GMPE_PPO_VALUENORM) {
        const float bm = (float)(sh[0][0] / n), bsq = (float)(sh[0][1] / n);
        const float rm = __fadd_rn(__fmul_rn(*p.rm, p.wbeta), __fmul_rn(bm, p.w1beta));       // running_mean.mul_(weight).add_(batch_mean * (1.0 - weight))
        const float rms = __fadd_rn(__fmul_rn(*p.rms, p.wbeta), __fmul_rn(bsq, p.w1beta));
        const float db = __fadd_rn(__fmul_rn(*p.db, p.wbeta), p.w1beta);
        *p.rm = rm; *p.rms = rms; *p.db = db;
        const float dc = fmaxf(db, p.eps);
        mean = __fdiv_rn(rm, dc);
        const float var = fmaxf(__fsub_rn(__fdiv_rn(rms, dc), __fmul_rn(mean, mean)), 1e-2f);
        sd = __fsqrt_rn(var);
    }
    float* f = reinterpret_cast<float*>(p.hdr + 2);
    f[0] = mean; f[1] = sd;
}

// 3: the row pass. One lane per row; the tile's available_actions, then its logits, then its gradient pass through the same LDS rows.
template <bool VEC, bool ACT64>
__global__ __launch_bounds__(TILE) void k_loss_rows(LossArgs p) {
    extern __shared__ __attribute__((aligned(16))) float sh[];
    __shared__ double red[NW * NROW];
    const int K = p.K, S = p.S;
    const int64_t row0 = (int64_t)blockIdx.x * TILE, r = row0 + threadIdx.x;
    const int rows = p.B - row0 < TILE ? (int)(p.B - row0) : TILE, n = rows * K;
    const bool live = (int)threadIdx.x < rows;
    float* row = sh + threadIdx.x * S;
    const int64_t g0 = row0 * K;

    uint64_t avail = ~0ull;
    if (p.avail) {
        tile_copy<VEC, true>(const_cast<float*>(p.avail) + g0, sh, n, K, S, p.magic);
        __syncthreads();
        if (live) avail = avail_bits(row, K);                                       // x[available_actions == 0] = finfo.min
        __syncthreads();
    }
    tile_copy<VEC, true>(const_cast<float*>(p.logits) + g0, sh, n, K, S, p.magic);
    __syncthreads();

    double acc[NROW] = {0.0, 0.0, 0.0, 0.0};
    if (live) {
        const double Dp = p.hdr[0], Dv = p.hdr[1];
        const float am = p.am[r];
        const float wp = (p.flags & GMPE_PPO_POLICY_ACTIVE_MASKS) ? am : 1.0f, wv = (p.flags & GMPE_PPO_VALUE_ACTIVE_MASKS) ? am : 1.0f;
        PolicyRow q;
        q.avail = avail;
        q.action = ACT64 ? static_cast<const int64_t*>(p.actions)[r] : (int64_t)static_cast<const float*>(p.actions)[r];   // .long() truncates
        q.adv = p.adv[r]; q.old_lp = p.old_lp[r]; q.wp = wp; q.Dp = (float)Dp; q.lo = p.lo; q.hi = p.hi; q.ent_coef = p.ent_coef;
        float la, ratio;
        policy_row(row, K, q, &la, &ratio, &acc[0], &acc[1]);
        acc[3] = (double)ratio;
        if (p.out_lp) p.out_lp[r] = la;
        if (p.out_ratio) p.out_ratio[r] = ratio;
        // ---- the value branch (graph_mappo.py:89-117)
        float R = p.ret[r];
        if (p.flags & GMPE_PPO_VALUENORM) {
            const float* st = reinterpret_cast<const float*>(p.hdr + 2);
            R = __fdiv_rn(__fsub_rn(R, st[0]), st[1]);
        }
        p.grad_values[r] = value_row<false>(p.values[r], p.vp[r], R, p.flags & GMPE_PPO_HUBER_LOSS, p.flags & GMPE_PPO_CLIPPED_VALUE_LOSS, p.clip, p.delta,
                                     p.half_delta, wv, (float)Dv, &acc[2]);
    }
    block_sum<NROW>(acc, red, p.row_part + (int64_t)blockIdx.x * NROW);     // its barrier also orders the gradient rows before the copy out
    tile_copy<VEC, false>(p.grad_logits + g0, sh, n, K, S, p.magic);
}

// 4: the partials -> the scalar row
__global__ __launch_bounds__(TILE) void k_loss_finish(LossArgs p, int64_t nparts) {
    __shared__ double sh[TILE][NROW];
    merge<NROW>(p.row_part, nparts, sh);
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
}

int64_t num_tiles(int64_t rows) { return (rows + TILE - 1) / TILE; }

int fail(int code, const std::string& m) { return gmpe::report_error(code, m); }

}  // namespace

#define LCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(GMPE_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

extern "C" {

int gmpe_ppo_loss_workspace_bytes(int64_t rows, size_t* bytes_out) {
    if (!bytes_out || rows < 1) return fail(GMPE_ERR_INVALID_ARG, "gmpe_ppo_loss_workspace_bytes: bad arguments");
    *bytes_out = ((size_t)num_tiles(rows) * (NSTAT + NROW) + HDR_DOUBLES) * sizeof(double);
    return GMPE_OK;
}

int gmpe_ppo_loss(int device, const gmpe_ppo_loss_plan* pl, void* stream) {
    if (!pl) return fail(GMPE_ERR_INVALID_ARG, "gmpe_ppo_loss: null plan");
    const int known = GMPE_PPO_POLICY_ACTIVE_MASKS | GMPE_PPO_VALUE_ACTIVE_MASKS | GMPE_PPO_CLIPPED_VALUE_LOSS | GMPE_PPO_HUBER_LOSS | GMPE_PPO_VALUENORM;
    if (pl->flags & ~known) return fail(GMPE_ERR_INVALID_ARG, "gmpe_ppo_loss: unknown flags");
    if (pl->rows < 1) return fail(GMPE_ERR_INVALID_ARG, "gmpe_ppo_loss: need rows >= 1");
    if (pl->n_actions < 1 || pl->n_actions > GMPE_PPO_MAX_ACTIONS)
        return fail(GMPE_ERR_INVALID_ARG, "gmpe_ppo_loss: n_actions must be in 1 .. " + std::to_string(GMPE_PPO_MAX_ACTIONS));
    if (pl->actions_int64 != 0 && pl->actions_int64 != 1) return fail(GMPE_ERR_INVALID_ARG, "gmpe_ppo_loss: actions_int64 must be 0 or 1");
    if (!pl->logits || !pl->values || !pl->actions || !pl->old_action_log_probs || !pl->adv_targ || !pl->value_preds || !pl->returns || !pl->active_masks)
        return fail(GMPE_ERR_INVALID_ARG, "gmpe_ppo_loss: logits, values, actions, old_action_log_probs, adv_targ, value_preds, returns and active_masks are required");
    if (!pl->out || !pl->grad_logits || !pl->grad_values) return fail(GMPE_ERR_INVALID_ARG, "gmpe_ppo_loss: out, grad_logits and grad_values are required");
    const bool vn = pl->flags & GMPE_PPO_VALUENORM;
    if (vn != (pl->running_mean && pl->running_mean_sq && pl->debiasing_term) || (!vn && (pl->running_mean || pl->running_mean_sq || pl->debiasing_term)))
        return fail(GMPE_ERR_INVALID_ARG, "gmpe_ppo_loss: the three ValueNorm scalars are given exactly with GMPE_PPO_VALUENORM");
    if (!(pl->clip_param >= 0.0) || !(pl->huber_delta >= 0.0) || !(pl->beta >= 0.0 && pl->beta <= 1.0) || !(pl->epsilon > 0.0) || pl->entropy_coef != pl->entropy_coef)
        return fail(GMPE_ERR_INVALID_ARG, "gmpe_ppo_loss: need clip_param >= 0, huber_delta >= 0, 0 <= beta <= 1, epsilon > 0 and a number for entropy_coef");
    const uintptr_t a4 = (uintptr_t)pl->logits | (uintptr_t)pl->available_actions | (uintptr_t)pl->values | (uintptr_t)pl->old_action_log_probs |
                         (uintptr_t)pl->adv_targ | (uintptr_t)pl->value_preds | (uintptr_t)pl->returns | (uintptr_t)pl->active_masks | (uintptr_t)pl->grad_logits |
                         (uintptr_t)pl->grad_values | (uintptr_t)pl->action_log_probs | (uintptr_t)pl->imp_weights | (uintptr_t)pl->running_mean |
                         (uintptr_t)pl->running_mean_sq | (uintptr_t)pl->debiasing_term;
    if ((a4 & 3) || ((uintptr_t)pl->actions & (pl->actions_int64 ? 7 : 3)) || ((uintptr_t)pl->out & 7))
        return fail(GMPE_ERR_INVALID_ARG, "gmpe_ppo_loss: f32 arrays must be 4-byte aligned, int64 actions and out 8-byte aligned");
    size_t need = 0;
    gmpe_ppo_loss_workspace_bytes(pl->rows, &need);
    if (!pl->workspace || pl->workspace_bytes < need || ((uintptr_t)pl->workspace & 7))
        return fail(GMPE_ERR_INVALID_ARG, "gmpe_ppo_loss: needs an 8-byte aligned workspace of gmpe_ppo_loss_workspace_bytes(rows)");
    const int64_t nt = num_tiles(pl->rows);
    if (nt > 0x7fffffffLL) return fail(GMPE_ERR_INVALID_ARG, "gmpe_ppo_loss: too many rows for one launch");
    LCHK(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    LossArgs a;
    a.B = pl->rows; a.K = pl->n_actions; a.S = pl->n_actions | 1; a.flags = pl->flags;
    a.magic = (uint32_t)(0x100000000ULL / (uint64_t)(pl->n_actions > 1 ? pl->n_actions : 2)) + 1u;
    a.logits = pl->logits; a.avail = pl->available_actions; a.values = pl->values; a.old_lp = pl->old_action_log_probs; a.adv = pl->adv_targ;
    a.vp = pl->value_preds; a.ret = pl->returns; a.am = pl->active_masks; a.actions = pl->actions;
    a.grad_logits = pl->grad_logits; a.grad_values = pl->grad_values; a.out_lp = pl->action_log_probs; a.out_ratio = pl->imp_weights;
    // a Python float meets a float32 tensor as float32(value): 1.0 - clip_param, 1.0 - beta and huber_delta / 2 are formed in double first
    a.lo = (float)(1.0 - pl->clip_param); a.hi = (float)(1.0 + pl->clip_param); a.clip = (float)pl->clip_param;
    a.delta = (float)pl->huber_delta; a.half_delta = (float)(pl->huber_delta / 2.0); a.ent_coef = (float)pl->entropy_coef;
    a.wbeta = (float)pl->beta; a.w1beta = (float)(1.0 - pl->beta); a.eps = (float)pl->epsilon;
    a.rm = pl->running_mean; a.rms = pl->running_mean_sq; a.db = pl->debiasing_term;
    a.stat_part = static_cast<double*>(pl->workspace);
    a.row_part = a.stat_part + nt * NSTAT;
    a.hdr = a.row_part + nt * NROW;
    a.out = pl->out;
    const dim3 grid((unsigned)nt), block(TILE), one(1);
    hipLaunchKernelGGL(k_loss_stats, grid, block, 0, st, a);
    LCHK(hipGetLastError());
    hipLaunchKernelGGL(k_loss_prepare, one, block, 0, st, a, nt);
    LCHK(hipGetLastError());
    const bool vec = !(((uintptr_t)pl->logits | (uintptr_t)pl->available_actions | (uintptr_t)pl->grad_logits) & 15);   // tiles start at multiples of 1 KiB
    const size_t lds = (size_t)TILE * a.S * sizeof(float);
    void (*fn)(LossArgs) = vec ? (pl->actions_int64 ? k_loss_rows<true, true> : k_loss_rows<true, false>)
                               : (pl->actions_int64 ? k_loss_rows<false, true> : k_loss_rows<false, false>);
    if (lds > 48 * 1024) {                                                    // K = 64 only; once per device and instantiation, at the largest size there is
        static std::atomic<bool> raised[64][4];
        const int v = (vec ? 2 : 0) | (pl->actions_int64 ? 1 : 0);
        if (device < 0 || device >= 64 || !raised[device][v].load()) {
            LCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)(TILE * (GMPE_PPO_MAX_ACTIONS | 1) * sizeof(float))));
            if (device >= 0 && device < 64) raised[device][v].store(true);
        }
    }
    hipLaunchKernelGGL(fn, grid, block, lds, st, a);
    LCHK(hipGetLastError());
    hipLaunchKernelGGL(k_loss_finish, one, block, 0, st, a, nt);
    LCHK(hipGetLastError());
    return GMPE_OK;
}

}  // extern "C"
