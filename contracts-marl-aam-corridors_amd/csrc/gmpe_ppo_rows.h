// gmpe_ppo_rows.h — the per-row arithmetic, the tile machinery and the fixed-order reductions of the row kernels over a policy head's logits, shared by
// gmpe_ppo_loss.hip (values in), gmpe_ppo_popart.hip (critic features in, PopArt), gmpe_act.hip (the rollout's action and log-prob) and gmpe_head.hip (the
// head's Linear in front of either): one text, so the entry points cannot drift apart — the log-prob the act kernel stores is the one the loss kernels recompute because both run the masked
// categorical below. Everything here is float32 per row in the reference's operation order (no contraction) and double across rows; the derivations of
// the gradients are at the head of gmpe_ppo_loss.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "gmpe_host.h"            // TILE, Geom

#pragma clang fp contract(off)

namespace gmpe_ppo {

constexpr int NW = TILE / 64;
constexpr int NSTAT = 3;          // sum returns, sum returns^2, sum active_masks
constexpr float FMIN = -FLT_MAX;  // torch.finfo(torch.float32).min

// lane 0 of every wave holds the wave's sum; the lower lane of a pair is the left operand (one fixed order)
template <int N>
__device__ __forceinline__ void wave_sum(double (&v)[N]) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const double o = __shfl_xor(v[k], off);
            v[k] = (threadIdx.x & off) ? o + v[k] : v[k] + o;
        }
    }
}

// the workgroup's sum of v[] -> dst[0..N), waves added in wave order
template <int N>
__device__ __forceinline__ void block_sum(double (&v)[N], double* red, double* dst) {
    wave_sum<N>(v);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < N; ++k) red[w * N + k] = v[k];
    __syncthreads();
    if (threadIdx.x < N) {
        double s = red[threadIdx.x];
        for (int q = 1; q < NW; ++q) s += red[q * N + threadIdx.x];
        dst[threadIdx.x] = s;
    }
}

// N columns of `part` [nparts, N] -> sh[0..N): thread i adds partials i, i + TILE, ... in order, then a fixed tree. The result depends on nparts alone.
template <int N>
__device__ __forceinline__ void merge(const double* __restrict__ part, int64_t nparts, double (*sh)[N]) {
    double s[N];
#pragma unroll
    for (int k = 0; k < N; ++k) s[k] = 0.0;
    for (int64_t i = threadIdx.x; i < nparts; i += TILE)
#pragma unroll
        for (int k = 0; k < N; ++k) s[k] += part[i * N + k];
#pragma unroll
    for (int k = 0; k < N; ++k) sh[threadIdx.x][k] = s[k];
    __syncthreads();
    for (int w = TILE / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
#pragma unroll
            for (int k = 0; k < N; ++k) sh[threadIdx.x][k] += sh[threadIdx.x + w][k];
        __syncthreads();
    }
}

// this workgroup's double sums of returns, returns^2, active_masks over its TILE rows -> stat_part[blockIdx.x]
__device__ __forceinline__ void stats_tile(const float* __restrict__ ret, const float* __restrict__ am, int64_t B, double* stat_part, double* red) {
    const int64_t r = (int64_t)blockIdx.x * TILE + threadIdx.x;
    double v[NSTAT] = {0.0, 0.0, 0.0};
    if (r < B) {
        const double x = ret[r];
        v[0] = x; v[1] = x * x; v[2] = am[r];
    }
    block_sum<NSTAT>(v, red, stat_part + (int64_t)blockIdx.x * NSTAT);
}

// A contiguous tile of n floats at g <-> its rows in LDS at stride S. VEC: 16-byte global accesses (g 16-byte aligned), else 4-byte ones.
// LDS side: with K odd S == K, the tile's LDS image is its global image and a lane's four floats move as one 16-byte access. With K even (S = K + 1) the
// four floats go one dword at a time; lane i starts at element (i / 8) % 4 of its four, so the lanes i, i + 8, i + 16, i + 24 of a 32-lane group, whose
// floats lie 32 dwords apart, are on four different banks in every round instead of on one.
template <bool VEC, bool IN>
__device__ __forceinline__ void tile_copy(float* g, float* sh, int n, int K, int S, uint32_t magic) {
    const int rot = (threadIdx.x >> 3) & 3;
    for (int f = threadIdx.x * 4; f < n; f += TILE * 4) {
        const int cnt = n - f < 4 ? n - f : 4;
        float v[4];
        if (IN) {
            if (VEC && cnt == 4) {
                const float4 t = *reinterpret_cast<const float4*>(g + f);
                v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < cnt) v[k] = g[f + k];
            }
        }
        if (S == K && cnt == 4) {
            float4* q = reinterpret_cast<float4*>(sh + f);
            if (IN) *q = make_float4(v[0], v[1], v[2], v[3]);
            else { const float4 t = *q; v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
        } else {
            const uint32_t r = K == 1 ? (uint32_t)f : __umulhi((uint32_t)f, magic);
            const uint32_t c = (uint32_t)f - r * (uint32_t)K;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int kk = (k + rot) & 3;
                uint32_t rr = r, cc = c + (uint32_t)kk;
                while (cc >= (uint32_t)K) { cc -= (uint32_t)K; ++rr; }
                if (kk < cnt) {
                    float* q = sh + rr * S + cc;
                    if (IN) *q = kk == 0 ? v[0] : (kk == 1 ? v[1] : (kk == 2 ? v[2] : v[3]));
                    else {
                        const float t = *q;
                        if (kk == 0) v[0] = t; else if (kk == 1) v[1] = t; else if (kk == 2) v[2] = t; else v[3] = t;
                    }
                }
            }
        }
        if (!IN) {
            if (VEC && cnt == 4) {
                *reinterpret_cast<float4*>(g + f) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < cnt) g[f + k] = v[k];
            }
        }
    }
}

// x[available_actions == 0] = finfo.min: the availability bits of this lane's row, read from the tile of available_actions in LDS
__device__ __forceinline__ uint64_t avail_bits(const float* row, int K) {
    uint64_t avail = 0;
    for (int j = 0; j < K; ++j) avail |= (uint64_t)(row[j] != 0.0f) << j;
    return avail;
}

// this lane's place in its workgroup's tile
struct Tile {
    int64_t row0, r, g0;           // the tile's first row, the lane's row; the tile's first float in a [B, K] array
    int rows, n;                   // rows and floats in the tile (the last tile may be short)
    bool live;                     // the lane has a row
    float* row;                    // the row in LDS
};

__device__ __forceinline__ Tile tile_of(const Geom& g, float* sh) {
    Tile t;
    t.row0 = (int64_t)blockIdx.x * TILE; t.r = t.row0 + threadIdx.x; t.g0 = t.row0 * g.K;
    t.rows = g.B - t.row0 < TILE ? (int)(g.B - t.row0) : TILE; t.n = t.rows * g.K;
    t.live = (int)threadIdx.x < t.rows; t.row = sh + threadIdx.x * g.S;
    return t;
}

// The head of a row kernel: the tile of available_actions (when given) passes through the LDS rows and leaves this lane's availability bits, else `avail`
// stays what the caller gave; then the tile of logits, behind a barrier.
template <bool VEC>
__device__ __forceinline__ uint64_t tile_in(const Geom& g, const Tile& t, const float* avail_g, const float* logits, float* sh, uint64_t avail) {
    if (avail_g) {
        tile_copy<VEC, true>(const_cast<float*>(avail_g) + t.g0, sh, t.n, g.K, g.S, g.magic);
        __syncthreads();
        if (t.live) avail = avail_bits(t.row, g.K);                                 // x[available_actions == 0] = finfo.min
        __syncthreads();
    }
    tile_copy<VEC, true>(const_cast<float*>(logits) + t.g0, sh, t.n, g.K, g.S, g.magic);
    __syncthreads();
    return avail;
}

// ---- the masked categorical (torch: logits - logsumexp, probs = softmax of that), in the three steps its users share
__device__ __forceinline__ float masked_logit(const float* row, uint64_t avail, int j) { return (avail >> j & 1) ? row[j] : FMIN; }

__device__ __forceinline__ float masked_max(const float* row, int K, uint64_t avail) {
    float m = -INFINITY;
    for (int j = 0; j < K; ++j) m = fmaxf(m, masked_logit(row, avail, j));
    return m;
}

__device__ __forceinline__ float exp_below(float l, float ml) { return expf(__fsub_rn(l, ml)); }

// m = masked_max of the row, which still holds the logits. On return the row holds l = x - logsumexp(x), Categorical's normalised logits; *ml = max_j l_j
// (rounding is monotone) and *s2 = sum_j exp(l_j - ml): torch renormalises the normalised logits, probs = softmax(l).
__device__ __forceinline__ void normalise_row(float* row, int K, uint64_t avail, float m, float* ml_out, float* s2_out) {
    float s = 0.0f;
    for (int j = 0; j < K; ++j) s = __fadd_rn(s, expf(__fsub_rn(masked_logit(row, avail, j), m)));
    const float lse = __fadd_rn(logf(s), m), ml = __fsub_rn(m, lse);
    float s2 = 0.0f;
    for (int j = 0; j < K; ++j) {
        const float l = __fsub_rn(masked_logit(row, avail, j), lse);
        row[j] = l;
        s2 = __fadd_rn(s2, exp_below(l, ml));
    }
    *ml_out = ml; *s2_out = s2;
}

// p_j of a normalised row
__device__ __forceinline__ float prob(float l, float ml, float s2) { return __fdiv_rn(exp_below(l, ml), s2); }

// what the policy side of a row needs besides its logits
struct PolicyRow {
    uint64_t avail;                // bit j: action j is available
    int64_t action;                // .long() of the stored action
    float adv, old_lp, wp;         // adv_targ, old_action_log_probs, the row's weight in the policy means (active_masks or 1)
    float Dp;                      // float32 of the policy denominator
    float lo, hi, ent_coef;        // 1 - clip, 1 + clip, entropy_coef
};

// The masked categorical, the ratio / clip / surrogate block and d actor_loss / d logits of one row. `row` holds the K logits on entry and the K
// gradients on return. acc0 = -min(surr1, surr2) * w, acc1 = H * w (the terms of the two means), la the action's log-prob, ratio the importance weight.
__device__ __forceinline__ void policy_row(float* row, int K, const PolicyRow& q, float* la_out, float* ratio_out, double* acc0, double* acc1) {
    const uint64_t avail = q.avail;
    float ml, s2;
    normalise_row(row, K, avail, masked_max(row, K, avail), &ml, &s2);
    const int64_t ai = q.action;
    const int a = ai < 0 ? 0 : (ai >= K ? K - 1 : (int)ai);                   // out of range is the caller's error (torch raises): stay inside the row
    const float la = row[a];
    float t = 0.0f;
    for (int j = 0; j < K; ++j) {
        const float l = row[j];
        t = __fadd_rn(t, __fmul_rn(fmaxf(l, FMIN), prob(l, ml, s2)));         // clamp(l, min=finfo.min) * p
    }
    const float H = -t;
    // ---- ratio, clip, surrogates (graph_mappo.py:176-197)
    const float adv = q.adv, wp = q.wp;
    const float ratio = expf(__fsub_rn(la, q.old_lp));
    const float surr1 = __fmul_rn(ratio, adv), surr2 = __fmul_rn(fminf(fmaxf(ratio, q.lo), q.hi), adv);
    const bool pass = surr1 < surr2 || (surr1 == surr2 && ratio >= q.lo && ratio <= q.hi);
    *acc0 = (double)__fmul_rn(-fminf(surr1, surr2), wp);
    *acc1 = (double)__fmul_rn(H, wp);
    *la_out = la;
    *ratio_out = ratio;
    const float cw = __fdiv_rn(wp, q.Dp);
    const float ca = pass ? -__fmul_rn(__fmul_rn(cw, adv), ratio) : 0.0f, ce = __fmul_rn(q.ent_coef, cw);
    for (int j = 0; j < K; ++j) {
        float g = 0.0f;
        if (avail >> j & 1) {
            const float l = row[j], pj = prob(l, ml, s2);
            g = __fadd_rn(__fmul_rn(ca, __fsub_rn(j == a ? 1.0f : 0.0f, pj)), __fmul_rn(ce, __fmul_rn(pj, __fadd_rn(l, H))));
        }
        row[j] = g;
    }
}

// what the policy side of the loss kernels' row pass reads and writes (both entry points embed it in their arguments)
struct PolicyArgs {
    const float *logits, *avail, *old_lp, *adv, *am;
    const void* actions;
    float *out_lp, *out_ratio;     // optional
    float lo, hi, ent_coef;        // 1 - clip, 1 + clip, entropy_coef
    int flags;                     // GMPE_PPO_*
};

// The policy side of row r: its weights from active_masks, policy_row over the row's logits in LDS (its gradients on return), the terms of the two means
// and of ratio_mean into acc[0], acc[1], acc[3], the two optional stores. Returns wv, the row's weight in the value mean. Dp: the policy denominator.
template <bool ACT64>
__device__ __forceinline__ float policy_side(const PolicyArgs& p, float* row, int K, int64_t r, uint64_t avail, double Dp, double* acc) {
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
    return wv;
}

// hdr[0], hdr[1]: the denominators of the policy means and of the value mean, from the merged sum of active_masks
__device__ __forceinline__ void denominators(double* hdr, int flags, int64_t B, double msum) {
    hdr[0] = (flags & GMPE_PPO_POLICY_ACTIVE_MASKS) ? msum : (double)B;
    hdr[1] = (flags & GMPE_PPO_VALUE_ACTIVE_MASKS) ? msum : (double)B;
}

// The running statistics of ValueNorm.update (valuenorm.py:56-73) and PopArt.update (popart.py:62-77), in place, float32, over all B rows (no mask):
// x.mul_(beta).add_(batch * (1.0 - beta)) for the mean and the mean of squares, debiasing_term.mul_(beta).add_(1.0 * (1.0 - beta)).
// sums: the merged double sums of returns and returns^2.
struct Running { float mean, mean_sq, debias; };
__device__ __forceinline__ Running running_update(float* mean, float* mean_sq, float* debias, const double* sums, int64_t B, float beta, float one_minus_beta) {
    const float bm = (float)(sums[0] / (double)B), bsq = (float)(sums[1] / (double)B);      // input_vector.mean(0), (input_vector ** 2).mean(0)
    Running u;
    u.mean = __fadd_rn(__fmul_rn(*mean, beta), __fmul_rn(bm, one_minus_beta));
    u.mean_sq = __fadd_rn(__fmul_rn(*mean_sq, beta), __fmul_rn(bsq, one_minus_beta));
    u.debias = __fadd_rn(__fmul_rn(*debias, beta), one_minus_beta);
    *mean = u.mean; *mean_sq = u.mean_sq; *debias = u.debias;
    return u;
}

// the seven scalars of a loss call from the merged row sums s[0..3] (the acc[] of the row pass)
__device__ __forceinline__ void write_scalars(double* out, const double* s, double Dp, double Dv, float ent_coef, int64_t B) {
    const double pol = s[0] / Dp, ent = s[1] / Dp;
    out[GMPE_PPO_OUT_POLICY_LOSS] = pol;
    out[GMPE_PPO_OUT_DIST_ENTROPY] = ent;
    out[GMPE_PPO_OUT_ACTOR_LOSS] = pol - (double)ent_coef * ent;
    out[GMPE_PPO_OUT_VALUE_LOSS] = s[2] / Dv;
    out[GMPE_PPO_OUT_RATIO_MEAN] = s[3] / (double)B;
    out[GMPE_PPO_OUT_DENOM_POLICY] = Dp;
    out[GMPE_PPO_OUT_DENOM_VALUE] = Dv;
}

__device__ __forceinline__ float value_term(float e, bool huber, float delta, float half_delta, float* dfde) {
    if (!huber) {                                               // mse_loss: e**2 / 2
        *dfde = e;
        return __fdiv_rn(__fmul_rn(e, e), 2.0f);
    }
    const float ae = fabsf(e);
    const float a = ae <= delta ? 1.0f : 0.0f, b = e > delta ? 1.0f : 0.0f;   // util.py:25-26: b = (e > d), one-sided
    *dfde = __fadd_rn(__fmul_rn(a, e), __fmul_rn(b, delta));
    return __fadd_rn(__fdiv_rn(__fmul_rn(a, __fmul_rn(e, e)), 2.0f), __fmul_rn(__fmul_rn(b, delta), __fsub_rn(ae, half_delta)));
}

// d (branch loss) / d e times the gradient cb that reaches the branch, formed as autograd forms it (huber: ((cb / 2) * a) * (2 * e) from a * e**2 / 2 plus
// (cb * (b * delta)) * sgn(e) from b * delta * (|e| - delta / 2); mse: (cb / 2) * (2 * e)). The factors are powers of two, a and b exclude each other, so a
// non-zero result has the bits of cb * f'(e); a zero result has autograd's sign.
__device__ __forceinline__ float value_term_grad(float cb, float e, bool huber, float delta) {
    const float h = __fmul_rn(cb, 0.5f), e2 = __fmul_rn(2.0f, e);
    if (!huber) return __fmul_rn(h, e2);
    const float a = fabsf(e) <= delta ? 1.0f : 0.0f, b = e > delta ? 1.0f : 0.0f;
    const float sg = e > 0.0f ? 1.0f : (e < 0.0f ? -1.0f : 0.0f);
    return __fadd_rn(__fmul_rn(__fmul_rn(h, a), e2), __fmul_rn(__fmul_rn(cb, __fmul_rn(b, delta)), sg));
}

// The value branch of one row (graph_mappo.py:89-117): v the critic's value, vp the stored prediction, R the (already normalised) return, wv the row's
// weight in the mean, Dv float32 of its denominator. Returns d value_loss / d v; *term = value_loss_row * wv.
// AUTOGRAD = false (gmpe_ppo_loss): the closed form w/D * g of the head of gmpe_ppo_loss.hip. AUTOGRAD = true (gmpe_ppo_loss_popart): the same number as
// the SUM autograd forms — torch.max hands the larger branch the whole incoming gradient, the smaller one +0 and each a half at a tie; the clipped branch's
// part passes the clamp only inside its range (+0 outside); the two parts are added. Every non-zero result has the closed form's bits; a zero (a masked row,
// the flat side of the one-sided huber) gets the sign the reference's .grad has, so g * W_j is the reference's grad_features bit for bit.
template <bool AUTOGRAD>
__device__ __forceinline__ float value_row(float v, float vp, float R, bool huber, bool clipped, float clip, float delta, float half_delta, float wv,
                                           float Dv, double* term) {
    const float d = __fsub_rn(v, vp);
    const float vpc = __fadd_rn(vp, fminf(fmaxf(d, -clip), clip));
    const float eo = __fsub_rn(R, v), ec = __fsub_rn(R, vpc);
    float fo, fc;
    const float Lo = value_term(eo, huber, delta, half_delta, &fo);
    const float Lc = value_term(ec, huber, delta, half_delta, &fc);
    const bool inside = d >= -clip && d <= clip;
    const float cw = __fdiv_rn(wv, Dv);
    if (AUTOGRAD) {
        if (!clipped) {
            *term = (double)__fmul_rn(Lo, wv);
            return -value_term_grad(cw, eo, huber, delta);
        }
        *term = (double)__fmul_rn(fmaxf(Lo, Lc), wv);
        const float half = __fmul_rn(cw, 0.5f);
        const float co = Lo > Lc ? cw : (Lc > Lo ? 0.0f : half), cc = Lc > Lo ? cw : (Lo > Lc ? 0.0f : half);
        return __fadd_rn(-value_term_grad(co, eo, huber, delta), inside ? -value_term_grad(cc, ec, huber, delta) : 0.0f);
    }
    const float go = -fo, gc = inside ? -fc : 0.0f;
    float L = Lo, g = go;
    if (clipped) {
        L = fmaxf(Lo, Lc);
        g = Lo > Lc ? go : (Lc > Lo ? gc : __fmul_rn(0.5f, __fadd_rn(go, gc)));
    }
    *term = (double)__fmul_rn(L, wv);
    return __fmul_rn(cw, g);
}

}  // namespace gmpe_ppo
