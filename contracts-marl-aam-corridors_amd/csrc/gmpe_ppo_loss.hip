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
// Over several shards (gmpe_ppo_loss_shard): the same kernels and the same host path (run_plan). LOCAL is the call up to k_loss_prepare, which writes the three
// sums and the row count to `local` instead of the header; APPLY starts at k_loss_prepare, which adds the shards' rows of `all` in index order instead of
// merging partials, and forms the denominators, the ValueNorm update and the normalisation scalars from the global sums: a shard's scalars are its sums over
// the global denominators, its gradient rows those of the global loss.
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

#include <string>

#include "gmpe_host.h"          // include/gmpe.h, the error text, GMPE_HIP_CHECK
#include "gmpe_ppo_rows.h"

#pragma clang fp contract(off)

namespace {

using namespace gmpe_ppo;         // gmpe_ppo_rows.h: TILE, the fixed-order sums, the tile machinery and the row arithmetic, shared with gmpe_ppo_popart.hip

constexpr int NROW = 4;           // sum -min(surr1, surr2) * w, sum H * w, sum value_loss * w, sum ratio
constexpr int HDR_DOUBLES = 4;    // D_policy, D_value, then f32 mean, std (one double), then the global row count of a sharded call
constexpr int NSHARD = GMPE_PPO_SHARD_STATS;      // the NSTAT sums and the row count

struct LossArgs {
    Geom g;
    PolicyArgs pol;
    const float *values, *vp, *ret;
    float *grad_logits, *grad_values;
    float clip, delta, half_delta, wbeta, w1beta, eps;
    float *rm, *rms, *db;
    double *stat_part, *row_part, *hdr, *out;
};

// 1: per-workgroup double sums of returns, returns^2, active_masks
__global__ __launch_bounds__(TILE) void k_loss_stats(LossArgs p) {
    __shared__ double red[NW * NSTAT];
    stats_tile(p.ret, p.pol.am, p.g.B, p.stat_part, red);
}

// 2: merge; ValueNorm.update (valuenorm.py:56-73), BEFORE the normalisation as cal_value_loss does (graph_mappo.py:93-97); running_mean_var (:48-54)
// sums: the merged sums of returns, returns^2, active_masks over the B rows the means are over (one thread)
__device__ __forceinline__ void prepare_header(const LossArgs& p, const double* sums, int64_t B) {
    denominators(p.hdr, p.pol.flags, B, sums[2]);
    float mean = 0.0f, sd = 1.0f;
    if (p.pol.flags & GMPE_PPO_VALUENORM) {
        const Running u = running_update(p.rm, p.rms, p.db, sums, B, p.wbeta, p.w1beta);
        const float dc = fmaxf(u.debias, p.eps);
        mean = __fdiv_rn(u.mean, dc);
        const float var = fmaxf(__fsub_rn(__fdiv_rn(u.mean_sq, dc), __fmul_rn(mean, mean)), 1e-2f);
        sd = __fsqrt_rn(var);
    }
    float* f = reinterpret_cast<float*>(p.hdr + 2);
    f[0] = mean; f[1] = sd;
}

// One kernel for the three callers. Source of the sums: `all` (gmpe_ppo_loss_shard, APPLY) = the shards' rows of NSHARD doubles added in index order by one
// thread (the order is the result), the row count with them; otherwise the merged partials of this call's rows and B. Sink: `local` (LOCAL) = the sums and the
// row count, and the kernel stops; otherwise hdr[3] = the row count, which k_loss_finish reads, and the header. The branch on `all` is uniform over the
// workgroup, so the barriers inside merge are reached by all of it or by none.
__global__ __launch_bounds__(TILE) void k_loss_prepare(LossArgs p, int64_t nparts, const double* __restrict__ all, int world, double* __restrict__ local) {
    __shared__ double sh[TILE][NSTAT];
    double s[NSHARD];
    if (all) {
        if (threadIdx.x != 0) return;
        for (int k = 0; k < NSHARD; ++k) s[k] = all[k];
        for (int i = 1; i < world; ++i)
            for (int k = 0; k < NSHARD; ++k) s[k] += all[i * NSHARD + k];
    } else {
        merge<NSTAT>(p.stat_part, nparts, sh);
        if (threadIdx.x != 0) return;
        for (int k = 0; k < NSTAT; ++k) s[k] = sh[0][k];
        s[NSTAT] = (double)p.g.B;
    }
    if (local) {
        for (int k = 0; k < NSHARD; ++k) local[k] = s[k];
        return;
    }
    p.hdr[3] = s[NSTAT];
    prepare_header(p, s, (int64_t)s[NSTAT]);
}

// 3: the row pass. One lane per row; the tile's available_actions, then its logits, then its gradient pass through the same LDS rows.
template <bool VEC, bool ACT64>
__global__ __launch_bounds__(TILE) void k_loss_rows(LossArgs p) {
    extern __shared__ __attribute__((aligned(16))) float sh[];
    __shared__ double red[NW * NROW];
    const Tile t = tile_of(p.g, sh);
    const uint64_t avail = tile_in<VEC>(p.g, t, p.pol.avail, p.pol.logits, sh, ~0ull);

    double acc[NROW] = {0.0, 0.0, 0.0, 0.0};
    if (t.live) {
        const int64_t r = t.r;
        const double Dp = p.hdr[0], Dv = p.hdr[1];
        const float wv = policy_side<ACT64>(p.pol, t.row, p.g.K, r, avail, Dp, acc);
        // ---- the value branch (graph_mappo.py:89-117)
        float R = p.ret[r];
        if (p.pol.flags & GMPE_PPO_VALUENORM) {
            const float* st = reinterpret_cast<const float*>(p.hdr + 2);
            R = __fdiv_rn(__fsub_rn(R, st[0]), st[1]);
        }
        p.grad_values[r] = value_row<false>(p.values[r], p.vp[r], R, p.pol.flags & GMPE_PPO_HUBER_LOSS, p.pol.flags & GMPE_PPO_CLIPPED_VALUE_LOSS, p.clip,
                                            p.delta, p.half_delta, wv, (float)Dv, &acc[2]);
    }
    block_sum<NROW>(acc, red, p.row_part + (int64_t)blockIdx.x * NROW);     // its barrier also orders the gradient rows before the copy out
    tile_copy<VEC, false>(p.grad_logits + t.g0, sh, t.n, p.g.K, p.g.S, p.g.magic);
}

// 4: the partials -> the scalar row: this call's sums over the denominators and the row count of the header (a shard's: the global ones)
__global__ __launch_bounds__(TILE) void k_loss_finish(LossArgs p, int64_t nparts) {
    __shared__ double sh[TILE][NROW];
    merge<NROW>(p.row_part, nparts, sh);
    if (threadIdx.x != 0) return;
    write_scalars(p.out, sh[0], p.hdr[0], p.hdr[1], p.pol.ent_coef, (int64_t)p.hdr[3]);
}

int fail(int code, const std::string& m) { return gmpe::report_error(code, m); }

// every check of a gmpe_ppo_loss_plan, for the entry point `name`
int check_plan(const char* name, const gmpe_ppo_loss_plan* pl) {
    const auto bad = [&](const char* m) { return fail(GMPE_ERR_INVALID_ARG, std::string(name) + ": " + m); };
    const int known = GMPE_PPO_POLICY_ACTIVE_MASKS | GMPE_PPO_VALUE_ACTIVE_MASKS | GMPE_PPO_CLIPPED_VALUE_LOSS | GMPE_PPO_HUBER_LOSS | GMPE_PPO_VALUENORM;
    if (pl->flags & ~known) return bad("unknown flags");
    const bool vn = pl->flags & GMPE_PPO_VALUENORM;
    const char* missing = nullptr;
    if (!pl->logits || !pl->values || !pl->actions || !pl->old_action_log_probs || !pl->adv_targ || !pl->value_preds || !pl->returns || !pl->active_masks)
        missing = "logits, values, actions, old_action_log_probs, adv_targ, value_preds, returns and active_masks are required";
    else if (!pl->out || !pl->grad_logits || !pl->grad_values)
        missing = "out, grad_logits and grad_values are required";
    else if (vn != (pl->running_mean && pl->running_mean_sq && pl->debiasing_term) || (!vn && (pl->running_mean || pl->running_mean_sq || pl->debiasing_term)))
        missing = "the three ValueNorm scalars are given exactly with GMPE_PPO_VALUENORM";
    if (int rc = check_loss_plan(name, pl, nullptr, missing)) return rc;
    const uintptr_t a4 = (uintptr_t)pl->logits | (uintptr_t)pl->available_actions | (uintptr_t)pl->values | (uintptr_t)pl->old_action_log_probs |
                         (uintptr_t)pl->adv_targ | (uintptr_t)pl->value_preds | (uintptr_t)pl->returns | (uintptr_t)pl->active_masks | (uintptr_t)pl->grad_logits |
                         (uintptr_t)pl->grad_values | (uintptr_t)pl->action_log_probs | (uintptr_t)pl->imp_weights | (uintptr_t)pl->running_mean |
                         (uintptr_t)pl->running_mean_sq | (uintptr_t)pl->debiasing_term;
    if ((a4 & 3) || ((uintptr_t)pl->actions & (pl->actions_int64 ? 7 : 3)) || ((uintptr_t)pl->out & 7))
        return bad("f32 arrays must be 4-byte aligned, int64 actions and out 8-byte aligned");
    size_t need = 0;
    gmpe_ppo_loss_workspace_bytes(pl->rows, &need);
    if (!pl->workspace || pl->workspace_bytes < need || ((uintptr_t)pl->workspace & 7))
        return bad("needs an 8-byte aligned workspace of gmpe_ppo_loss_workspace_bytes(rows)");
    if (num_tiles(pl->rows) > 0x7fffffffLL) return bad("too many rows for one launch");
    return GMPE_OK;
}

LossArgs loss_args(const gmpe_ppo_loss_plan* pl, int64_t nt) {
    LossArgs a;
    a.g = geometry(pl->rows, pl->n_actions);
    a.pol.flags = pl->flags;
    a.pol.logits = pl->logits; a.pol.avail = pl->available_actions; a.values = pl->values; a.pol.old_lp = pl->old_action_log_probs; a.pol.adv = pl->adv_targ;
    a.vp = pl->value_preds; a.ret = pl->returns; a.pol.am = pl->active_masks; a.pol.actions = pl->actions;
    a.grad_logits = pl->grad_logits; a.grad_values = pl->grad_values; a.pol.out_lp = pl->action_log_probs; a.pol.out_ratio = pl->imp_weights;
    hyper_parameters(pl, a);
    a.rm = pl->running_mean; a.rms = pl->running_mean_sq; a.db = pl->debiasing_term;
    a.stat_part = static_cast<double*>(pl->workspace);
    a.row_part = a.stat_part + nt * NSTAT;
    a.hdr = a.row_part + nt * NROW;
    a.out = pl->out;
    return a;
}

// the row pass of a plan: one launch
int launch_rows(const gmpe_ppo_loss_plan* pl, const LossArgs& a, int64_t nt, int device, hipStream_t st) {
    const bool vec = !(((uintptr_t)pl->logits | (uintptr_t)pl->available_actions | (uintptr_t)pl->grad_logits) & 15);   // tiles start at multiples of 1 KiB
    const size_t lds = (size_t)TILE * a.g.S * sizeof(float);
    void (*fn)(LossArgs) = vec ? (pl->actions_int64 ? k_loss_rows<true, true> : k_loss_rows<true, false>)
                               : (pl->actions_int64 ? k_loss_rows<false, true> : k_loss_rows<false, false>);
    if (lds > 48 * 1024)                                                      // K = 64 only
        if (int rc = gmpe::raise_dynamic_lds_once(reinterpret_cast<const void*>(fn), device, (vec ? 2 : 0) | (pl->actions_int64 ? 1 : 0),
                                            TILE * (GMPE_PPO_MAX_ACTIONS | 1) * sizeof(float)))
            return rc;
    hipLaunchKernelGGL(fn, dim3((unsigned)nt), dim3(TILE), lds, st, a);
    GMPE_HIP_CHECK(hipGetLastError());
    return GMPE_OK;
}

// A checked plan, for both entry points: the statistics unless the shards' are given (`all`), prepare, and the row pass with the scalars unless the
// statistics are all that is asked for (`local`). (null, 0, null) is the unsharded call: 4 launches; LOCAL 2, APPLY 3.
int run_plan(int device, const gmpe_ppo_loss_plan* pl, void* stream, const double* all, int world, double* local) {
    const int64_t nt = num_tiles(pl->rows);
    GMPE_HIP_CHECK(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const LossArgs a = loss_args(pl, nt);
    const dim3 grid((unsigned)nt), block(TILE), one(1);
    if (!all) {
        hipLaunchKernelGGL(k_loss_stats, grid, block, 0, st, a);
        GMPE_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_loss_prepare, one, block, 0, st, a, nt, all, world, local);
    GMPE_HIP_CHECK(hipGetLastError());
    if (local) return GMPE_OK;
    if (int rc = launch_rows(pl, a, nt, device, st)) return rc;
    hipLaunchKernelGGL(k_loss_finish, one, block, 0, st, a, nt);
    GMPE_HIP_CHECK(hipGetLastError());
    return GMPE_OK;
}

}  // namespace

extern "C" {

int gmpe_ppo_loss_workspace_bytes(int64_t rows, size_t* bytes_out) {
    if (!bytes_out || rows < 1) return fail(GMPE_ERR_INVALID_ARG, "gmpe_ppo_loss_workspace_bytes: bad arguments");
    *bytes_out = ((size_t)num_tiles(rows) * (NSTAT + NROW) + HDR_DOUBLES) * sizeof(double);
    return GMPE_OK;
}

int gmpe_ppo_loss(int device, const gmpe_ppo_loss_plan* pl, void* stream) {
    if (!pl) return fail(GMPE_ERR_INVALID_ARG, "gmpe_ppo_loss: null plan");
    if (int rc = check_plan("gmpe_ppo_loss", pl)) return rc;
    return run_plan(device, pl, stream, nullptr, 0, nullptr);
}

int gmpe_ppo_loss_shard(int device, const gmpe_ppo_loss_shard_plan* sp, void* stream) {
    if (!sp) return fail(GMPE_ERR_INVALID_ARG, "gmpe_ppo_loss_shard: null plan");
    if (int rc = gmpe::check_shard_args("gmpe_ppo_loss_shard", sp->phase, sp->world, sp->local, sp->all)) return rc;
    if (int rc = check_plan("gmpe_ppo_loss_shard", &sp->base)) return rc;
    const bool local = sp->phase == GMPE_SHARD_LOCAL;
    return run_plan(device, &sp->base, stream, local ? nullptr : sp->all, (int)sp->world, local ? sp->local : nullptr);
}

}  // extern "C"
