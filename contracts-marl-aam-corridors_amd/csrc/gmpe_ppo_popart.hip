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

#include <string>

#include "gmpe_host.h"          // include/gmpe.h, the error text, GMPE_HIP_CHECK
#include "gmpe_ppo_rows.h"

#pragma clang fp contract(off)

namespace {

using namespace gmpe_ppo;

constexpr int NROWP = 5;          // sum -min(surr1, surr2) * w, sum H * w, sum value_loss * w, sum ratio, sum g (d value_loss / d bias)
constexpr int HDR_DOUBLES = 8;    // D_policy, D_value, then f32: mean_d, sd, stddev, stddev', b' (three doubles), the rest spare
constexpr int MAXQ = GMPE_POPART_MAX_HIDDEN / 4 / 64;   // quads per lane and row at the largest H
constexpr int FIN_COLS = 16, FIN_SLICES = TILE / FIN_COLS;   // finish: 16 columns per workgroup, 16 slices of the partials per column
static_assert(MAXQ == 4, "the feature mapping holds at most four quads per lane");

struct PopArgs {
    Geom g;
    PolicyArgs pol;
    int H, NQ, L, lsh, vecf;       // NQ = ceil(H / 4); L = 1 << lsh lanes per row; vecf: features and grad_features move in 16-byte units
    const float *feat, *W, *bias, *stddev, *vp, *ret;
    float *grad_logits, *grad_feat, *grad_W, *grad_b, *values_out, *W_out, *bias_out, *stddev_out;
    float clip, delta, half_delta, wbeta, w1beta, eps;
    float *mean, *mean_sq, *db;
    double *stat_part, *row_part, *col_part, *hdr, *out;
};

// torch.clamp(x, min=lo): NaN stays NaN (fmaxf would return lo)
__device__ __forceinline__ float clamp_min(float x, float lo) { return x != x ? x : fmaxf(x, lo); }

// 1: per-workgroup double sums of returns, returns^2, active_masks
__global__ __launch_bounds__(TILE) void k_pop_stats(PopArgs p) {
    __shared__ double red[NW * NSTAT];
    stats_tile(p.ret, p.pol.am, p.g.B, p.stat_part, red);
}

// 2: merge; PopArt.update (popart.py:62-83) BEFORE normalize, as cal_value_loss does. The new weight is left to `finish`; stddev' and b' wait in the header.
__global__ __launch_bounds__(TILE) void k_pop_prepare(PopArgs p, int64_t nparts) {
    __shared__ double sh[TILE][NSTAT];
    merge<NSTAT>(p.stat_part, nparts, sh);
    if (threadIdx.x != 0) return;
    denominators(p.hdr, p.pol.flags, p.g.B, sh[0][2]);
    const float s_old = *p.stddev, b = *p.bias;                                              // old_stddev; old_mean is NOT kept: it aliases self.mean
    const Running u = running_update(p.mean, p.mean_sq, p.db, sh[0], p.g.B, p.wbeta, p.w1beta);
    const float mean = u.mean, msq = u.mean_sq, db = u.debias;
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
    const int H = p.H, NQ = p.NQ, L = p.L;
    const Tile t = tile_of(p.g, sh);
    const int64_t row0 = t.row0;
    const int rows = t.rows;
    double* colsum = reinterpret_cast<double*>(sh + ((TILE * p.g.S + 3) & ~3));
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
    const uint64_t avail = tile_in<VEC>(p.g, t, p.pol.avail, p.pol.logits, sh, ~0ull);      // its last barrier also orders vsh

    double acc[NROWP] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (t.live) {
        const int64_t r = t.r;
        const double Dp = p.hdr[0], Dv = p.hdr[1];
        const float wv = policy_side<ACT64>(p.pol, t.row, p.g.K, r, avail, Dp, acc);
        const float v = vsh[threadIdx.x];
        if (p.values_out) p.values_out[r] = v;
        const float* st = reinterpret_cast<const float*>(p.hdr + 2);
        const float R = __fdiv_rn(__fsub_rn(p.ret[r], st[0]), st[1]);       // normalize: (returns - mean_d) / sqrt(var_d)
        const float g = value_row<true>(v, p.vp[r], R, p.pol.flags & GMPE_PPO_HUBER_LOSS, p.pol.flags & GMPE_PPO_CLIPPED_VALUE_LOSS, p.clip, p.delta, p.half_delta, wv,
                                  (float)Dv, &acc[2]);
        gsh[threadIdx.x] = g;
        acc[4] = (double)g;
    }
    block_sum<NROWP>(acc, red, p.row_part + (int64_t)blockIdx.x * NROWP);    // its barrier also orders gsh and the gradient rows before the copy out
    tile_copy<VEC, false>(p.grad_logits + t.g0, sh, t.n, p.g.K, p.g.S, p.g.magic);

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
        write_scalars(p.out, sh[0], p.hdr[0], p.hdr[1], p.pol.ent_coef, p.g.B);
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

int fail(int code, const std::string& m) { return gmpe::report_error(code, m); }

}  // namespace

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
    const bool bad_hidden = pl->hidden < 1 || pl->hidden > GMPE_POPART_MAX_HIDDEN;
    const std::string dims = bad_hidden ? "hidden must be in 1 .. " + std::to_string(GMPE_POPART_MAX_HIDDEN) : std::string();
    const char* missing = nullptr;
    if (!pl->logits || !pl->critic_features || !pl->actions || !pl->old_action_log_probs || !pl->adv_targ || !pl->value_preds || !pl->returns ||
        !pl->active_masks)
        missing = "logits, critic_features, actions, old_action_log_probs, adv_targ, value_preds, returns and active_masks are required";
    else if (!pl->weight || !pl->bias || !pl->stddev || !pl->mean || !pl->mean_sq || !pl->debiasing_term || !pl->weight_out || !pl->bias_out || !pl->stddev_out)
        missing = "weight, bias, stddev, mean, mean_sq, debiasing_term, weight_out, bias_out and stddev_out are required";
    else if (!pl->out || !pl->grad_logits || !pl->grad_features || !pl->grad_weight || !pl->grad_bias)
        missing = "out, grad_logits, grad_features, grad_weight and grad_bias are required";
    if (int rc = check_loss_plan("gmpe_ppo_loss_popart", pl, bad_hidden ? dims.c_str() : nullptr, missing)) return rc;
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
    GMPE_HIP_CHECK(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    PopArgs a;
    a.g = geometry(pl->rows, pl->n_actions);
    a.pol.flags = pl->flags;
    a.H = pl->hidden; a.NQ = (pl->hidden + 3) / 4;
    a.lsh = 0;
    while ((1 << a.lsh) < a.NQ && a.lsh < 6) ++a.lsh;
    a.L = 1 << a.lsh;
    a.vecf = pl->hidden % 4 == 0 && !(((uintptr_t)pl->critic_features | (uintptr_t)pl->grad_features) & 15);
    a.pol.logits = pl->logits; a.pol.avail = pl->available_actions; a.feat = pl->critic_features; a.W = pl->weight; a.bias = pl->bias; a.stddev = pl->stddev;
    a.pol.old_lp = pl->old_action_log_probs; a.pol.adv = pl->adv_targ; a.vp = pl->value_preds; a.ret = pl->returns; a.pol.am = pl->active_masks;
    a.pol.actions = pl->actions;
    a.grad_logits = pl->grad_logits; a.grad_feat = pl->grad_features; a.grad_W = pl->grad_weight; a.grad_b = pl->grad_bias; a.values_out = pl->values_out;
    a.pol.out_lp = pl->action_log_probs; a.pol.out_ratio = pl->imp_weights; a.W_out = pl->weight_out; a.bias_out = pl->bias_out; a.stddev_out = pl->stddev_out;
    hyper_parameters(pl, a);
    a.mean = pl->mean; a.mean_sq = pl->mean_sq; a.db = pl->debiasing_term;
    a.stat_part = static_cast<double*>(pl->workspace);
    a.row_part = a.stat_part + nt * NSTAT;
    a.hdr = a.row_part + nt * NROWP;
    a.col_part = a.hdr + HDR_DOUBLES;
    a.out = pl->out;
    const dim3 grid((unsigned)nt), block(TILE), one(1);
    hipLaunchKernelGGL(k_pop_stats, grid, block, 0, st, a);
    GMPE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_pop_prepare, one, block, 0, st, a, nt);
    GMPE_HIP_CHECK(hipGetLastError());
    const bool vec = !(((uintptr_t)pl->logits | (uintptr_t)pl->available_actions | (uintptr_t)pl->grad_logits) & 15);   // tiles start at multiples of 1 KiB
    const size_t lds = (size_t)((TILE * a.g.S + 3) & ~3) * sizeof(float) + (size_t)4 * a.L * MAXQ * sizeof(double);
    void (*fn)(PopArgs) = vec ? (pl->actions_int64 ? k_pop_rows<true, true> : k_pop_rows<true, false>)
                              : (pl->actions_int64 ? k_pop_rows<false, true> : k_pop_rows<false, false>);
    if (lds > 48 * 1024)                                                      // large K or H
        if (int rc = gmpe::raise_dynamic_lds_once(reinterpret_cast<const void*>(fn), device, (vec ? 2 : 0) | (pl->actions_int64 ? 1 : 0),
                                            ((TILE * (GMPE_PPO_MAX_ACTIONS | 1) + 3) & ~3) * sizeof(float) + 4 * 64 * MAXQ * sizeof(double)))
            return rc;
    hipLaunchKernelGGL(fn, grid, block, lds, st, a);
    GMPE_HIP_CHECK(hipGetLastError());
    const dim3 fin(1 + (unsigned)((pl->hidden + FIN_COLS - 1) / FIN_COLS));
    hipLaunchKernelGGL(k_pop_finish, fin, block, 0, st, a, nt);
    GMPE_HIP_CHECK(hipGetLastError());
    return GMPE_OK;
}

}  // extern "C"
