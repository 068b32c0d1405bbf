// gmpe_returns.hip — learner side of a rollout: returns, advantages and the stop-action rows of available_actions (include/gmpe.h
// gmpe_compute_returns / gmpe_available_actions_from_dones). Handle-less: the learner may own no envs.
//
// Returns (GraphReplayBuffer.compute_returns, onpolicy/utils/graph_buffer.py:285-366): one lane per (env, agent), a reverse loop over
// t. The loads of a step do not depend on the recurrence, so each lane loads CH steps of every input at once and then runs the dependent
// chain over them: at c3 only 640 waves exist and a load per step would pay one memory latency per step.
// Bitwise parity with the reference's float32 NumPy: every product / sum below is the reference's own, in its order (Python evaluates
// `a + b * c * d - e` as (a + ((b * c) * d)) - e, a Python float meets a float32 array as float32(value)), no contraction, and the
// GAE factor is float32(gamma * gae_lambda) rounded from the double product Python forms first. ValueNorm.denormalize is torch's
// x * std then + mean: two roundings.
//
// Normalised advantages (GR_MAPPO.train, graph_mappo.py:294-304): each wave merges its lanes' (count, mean, M2) in double (Welford per
// lane, Chan merges in a fixed butterfly order) into one partial; k_adv_stats merges the partials in a fixed order; k_adv_normalize
// applies (adv - mean) / (std + 1e-5). No atomics: bitwise reproducible run to run.
//
// Over several shards (gmpe_compute_returns_shard): the same kernels and the same host path (run_plan). LOCAL is the call up to k_adv_stats, which writes the
// merged Stat itself to `local`; APPLY starts at k_adv_stats, which folds the shards' Stats of `all` with the same chan from the left in index order instead of
// merging partials, and normalises. The statistics are those of the whole batch, the same bits on every shard; with one shard LOCAL + APPLY is
// gmpe_compute_returns bit for bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "gmpe_host.h"          // include/gmpe.h, the error text, GMPE_HIP_CHECK

#pragma clang fp contract(off)

namespace {

constexpr int RET_BLOCK = 64;     // one wave per workgroup: the c3 grid (640 waves) spreads over every CU
constexpr int CH = 8;             // steps loaded ahead of the recurrence
constexpr int STAT_BLOCK = 256;
constexpr int NORM_BLOCK = 256;
constexpr int AVAIL_BLOCK = 256;

struct Stat { double n, mean, m2; };

__device__ __forceinline__ void welford(Stat& s, float xf) {
    const double x = xf;
    s.n += 1.0;
    const double d = x - s.mean;
    s.mean += d / s.n;
    s.m2 += d * (x - s.mean);
}

// Chan et al. merge, a before b (the order is part of the result: callers keep it fixed)
__device__ __forceinline__ Stat chan(const Stat& a, const Stat& b) {
    if (b.n == 0.0) return a;
    if (a.n == 0.0) return b;
    const double n = a.n + b.n, f = b.n / n, d = b.mean - a.mean;
    return Stat{n, a.mean + d * f, a.m2 + b.m2 + d * d * (a.n * f)};
}

struct RetArgs {
    int T;
    int64_t lanes, stride;
    float g, gl;                   // float32(gamma), float32(gamma * gae_lambda)
    const float *rew, *masks, *bad, *nv, *mu, *sd, *am;
    float *vp, *ret, *adv;         // adv: raw advantages (the normalised output when only that is asked for), or null
    Stat* part;                    // per-wave partials, or null (no statistics)
};

__device__ __forceinline__ float denorm(float x, float sd, float mu) { return __fadd_rn(__fmul_rn(x, sd), mu); }

__device__ __forceinline__ void wave_partial(Stat s, Stat* part) {
    // butterfly over the 64 lanes; the lower lane of every pair is the left operand, so lane 0's result has one fixed merge order
    const int lane = threadIdx.x;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const Stat o{__shfl_xor(s.n, off), __shfl_xor(s.mean, off), __shfl_xor(s.m2, off)};
        s = (lane & off) ? chan(o, s) : chan(s, o);
    }
    if (lane == 0) part[blockIdx.x] = s;
}

// One lane per (env, agent). GAE / PROPER / DN: the branch of compute_returns and whether a normaliser denormalises.
template <bool GAE, bool PROPER, bool DN>
__global__ __launch_bounds__(RET_BLOCK) void k_returns(RetArgs p) {
    const int64_t q = (int64_t)blockIdx.x * RET_BLOCK + threadIdx.x;
    Stat st{0.0, 0.0, 0.0};
    if (q < p.lanes) {
        const float sd = DN ? *p.sd : 1.0f, mu = DN ? *p.mu : 0.0f;
        const int64_t S = p.stride;
        const bool need_v = GAE || PROPER || p.adv;
        const float nv = p.nv[q];
        float gae = 0.0f, v1d = 0.0f, r1 = 0.0f;   // GAE: the (denormalised) value of step t + 1; otherwise returns[t + 1]
        if (GAE) {
            p.vp[(int64_t)p.T * S + q] = nv;         // self.value_preds[-1] = next_value
            v1d = DN ? denorm(nv, sd, mu) : nv;
        } else {
            p.ret[(int64_t)p.T * S + q] = nv;        // self.returns[-1] = next_value
            r1 = nv;
        }
        for (int hi = p.T; hi > 0; hi -= CH) {
            float r[CH], m1[CH], b1[CH], v0[CH], am[CH];
#pragma unroll
            for (int k = 0; k < CH; ++k) {
                const int t = hi - 1 - k;
                if (t < 0) break;
                const int64_t o = (int64_t)t * S + q;
                r[k] = p.rew[o];
                m1[k] = p.masks[o + S];
                if (PROPER) b1[k] = p.bad[o + S];
                if (need_v) v0[k] = p.vp[o];
                if (p.part) am[k] = p.am[o];
            }
#pragma unroll
            for (int k = 0; k < CH; ++k) {
                const int t = hi - 1 - k;
                if (t < 0) break;
                const float v0d = DN ? denorm(v0[k], sd, mu) : v0[k];
                float R;
                if (GAE) {
                    const float delta = __fsub_rn(__fadd_rn(r[k], __fmul_rn(__fmul_rn(p.g, v1d), m1[k])), v0d);
                    // with a normaliser and proper time limits the reference writes gamma * gae_lambda * gae * masks (graph_buffer.py:310-311)
                    gae = __fadd_rn(delta, (PROPER && DN) ? __fmul_rn(__fmul_rn(p.gl, gae), m1[k]) : __fmul_rn(__fmul_rn(p.gl, m1[k]), gae));
                    if (PROPER) gae = __fmul_rn(gae, b1[k]);
                    R = __fadd_rn(gae, v0d);
                    v1d = v0d;
                } else {
                    R = __fadd_rn(__fmul_rn(__fmul_rn(r1, p.g), m1[k]), r[k]);
                    if (PROPER) R = __fadd_rn(__fmul_rn(R, b1[k]), __fmul_rn(__fsub_rn(1.0f, b1[k]), v0d));
                    r1 = R;
                }
                const int64_t o = (int64_t)t * S + q;
                p.ret[o] = R;
                if (p.adv) {
                    const float a = __fsub_rn(R, v0d);     // buffer.returns[:-1] - denormalize(buffer.value_preds[:-1])
                    p.adv[o] = a;
                    if (p.part && am[k] != 0.0f && a == a) welford(st, a);   // active_masks == 0 -> NaN, then np.nan* skip NaNs
                }
            }
        }
    }
    if (p.part) wave_partial(st, p.part);
}

// GR_MAPPO.train's advantages from the returns / value_preds as they stand (no recurrence).
template <bool DN>
__global__ __launch_bounds__(RET_BLOCK) void k_advantages(RetArgs p) {
    const int64_t q = (int64_t)blockIdx.x * RET_BLOCK + threadIdx.x;
    Stat st{0.0, 0.0, 0.0};
    if (q < p.lanes) {
        const float sd = DN ? *p.sd : 1.0f, mu = DN ? *p.mu : 0.0f;
        const int64_t S = p.stride;
        for (int lo = 0; lo < p.T; lo += CH) {
            float R[CH], v0[CH], am[CH];
#pragma unroll
            for (int k = 0; k < CH; ++k) {
                if (lo + k >= p.T) break;
                const int64_t o = (int64_t)(lo + k) * S + q;
                R[k] = p.ret[o];
                v0[k] = p.vp[o];
                if (p.part) am[k] = p.am[o];
            }
#pragma unroll
            for (int k = 0; k < CH; ++k) {
                if (lo + k >= p.T) break;
                const float a = __fsub_rn(R[k], DN ? denorm(v0[k], sd, mu) : v0[k]);
                p.adv[(int64_t)(lo + k) * S + q] = a;
                if (p.part && am[k] != 0.0f && a == a) welford(st, a);
            }
        }
    }
    if (p.part) wave_partial(st, p.part);
}

// The partials in a fixed order -> sh[0] (every thread of the workgroup calls it; thread 0 reads the result)
__device__ __forceinline__ void merge_partials(const Stat* __restrict__ part, int64_t nparts, Stat* sh) {
    Stat s{0.0, 0.0, 0.0};
    for (int64_t i = threadIdx.x; i < nparts; i += STAT_BLOCK) s = chan(s, part[i]);
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = STAT_BLOCK / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] = chan(sh[threadIdx.x], sh[threadIdx.x + w]);
        __syncthreads();
    }
}

// A merged Stat -> mean, std + 1e-5 as float32 (np.nanmean / np.nanstd, ddof 0). No active entry: NaN, like NumPy.
__device__ __forceinline__ void mean_and_denominator(const Stat& t, float* __restrict__ out) {
    if (t.n == 0.0) {
        out[0] = out[1] = __builtin_nanf("");
    } else {
        out[0] = (float)t.mean;
        out[1] = __fadd_rn((float)sqrt(fmax(t.m2, 0.0) / t.n), 1e-5f);   // std_advantages + 1e-5 (float32 scalar arithmetic)
    }
}

// One kernel for the three callers. Source of the Stat: `all` (gmpe_compute_returns_shard, APPLY) = the shards' (n, mean, M2) as a left fold in index order
// by one thread (the order is the result); otherwise this call's partials. Sink: `local` (LOCAL) = the Stat itself; otherwise (mean, std + 1e-5) to `out`.
// The branch on `all` is uniform over the workgroup, so the barriers inside merge_partials are reached by all of it or by none.
__global__ __launch_bounds__(STAT_BLOCK) void k_adv_stats(const Stat* __restrict__ part, int64_t nparts, const double* __restrict__ all, int world,
                                                          double* __restrict__ local, float* __restrict__ out) {
    __shared__ Stat sh[STAT_BLOCK];
    Stat s;
    if (all) {
        if (threadIdx.x != 0) return;
        s = Stat{all[0], all[1], all[2]};
        for (int i = 1; i < world; ++i) s = chan(s, Stat{all[3 * i], all[3 * i + 1], all[3 * i + 2]});
    } else {
        merge_partials(part, nparts, sh);
        if (threadIdx.x != 0) return;
        s = sh[0];
    }
    if (local) {
        local[0] = s.n; local[1] = s.mean; local[2] = s.m2;
    } else {
        mean_and_denominator(s, out);
    }
}

__global__ __launch_bounds__(NORM_BLOCK) void k_adv_normalize(const float* src, float* dst, const float* __restrict__ stats, int T, int64_t lanes,
                                                             int64_t stride) {
    const int64_t q = (int64_t)blockIdx.x * NORM_BLOCK + threadIdx.x;
    if (q >= lanes) return;
    const float mean = stats[0], den = stats[1];
    for (int lo = 0; lo < T; lo += CH) {
        float a[CH];
#pragma unroll
        for (int k = 0; k < CH; ++k)
            if (lo + k < T) a[k] = src[(int64_t)(lo + k) * stride + q];
#pragma unroll
        for (int k = 0; k < CH; ++k)
            if (lo + k < T) dst[(int64_t)(lo + k) * stride + q] = __fdiv_rn(__fsub_rn(a[k], mean), den);
    }
}

// One thread per output float of a position's [lanes, n_actions] rows (coalesced stores); blockIdx.y = the step.
__global__ __launch_bounds__(AVAIL_BLOCK) void k_stop_actions(const uint8_t* __restrict__ dones, float* __restrict__ out, uint32_t per_pos, uint32_t n,
                                                             int T, int first, int64_t sd, int64_t so) {
    const uint32_t e = blockIdx.x * AVAIL_BLOCK + threadIdx.x;
    if (e >= per_pos) return;
    const int t = (first + (int)blockIdx.y) % T;
    const uint32_t lane = e / n, j = e - lane * n;
    float v = 1.0f;
    if (t > 0 && dones[(int64_t)(t - 1) * sd + lane]) v = j == n / 2 ? 1.0f : 0.0f;   // available_actions[int(n / 2)] = 1
    out[(int64_t)t * so + e] = v;
}

int64_t num_partials(int64_t lanes) { return (lanes + RET_BLOCK - 1) / RET_BLOCK; }

int fail(int code, const std::string& m) { return gmpe::report_error(code, m); }

// The checks of gmpe_compute_returns (stats: whether the statistics are needed, which a sharded call always does); `name` is the entry point's.
int check_returns_plan(const char* name, const gmpe_returns_plan* pl, bool stats) {
    const auto bad = [&](const char* m) { return fail(GMPE_ERR_INVALID_ARG, std::string(name) + ": " + m); };
    const bool proper = pl->flags & GMPE_RETURNS_PROPER_TIME_LIMITS, only = pl->flags & GMPE_RETURNS_ADVANTAGES_ONLY;
    if (pl->flags & ~(GMPE_RETURNS_GAE | GMPE_RETURNS_PROPER_TIME_LIMITS | GMPE_RETURNS_ADVANTAGES_ONLY)) return bad("unknown flags");
    if (pl->num_steps < 1 || pl->lanes < 1 || pl->stride < pl->lanes) return bad("need num_steps >= 1, lanes >= 1 and stride >= lanes");
    if (!pl->value_preds || !pl->returns) return bad("value_preds and returns are required");
    if (!only && (!pl->rewards || !pl->masks || !pl->next_value)) return bad("rewards, masks and next_value are required");
    if (!only && proper && !pl->bad_masks) return bad("proper time limits need bad_masks");
    if (!pl->denorm_mean != !pl->denorm_std) return bad("denorm_mean and denorm_std go together");
    if (only && !pl->advantages && !pl->normalized) return bad("advantages-only needs advantages or normalized");
    size_t need = 0;
    gmpe_returns_workspace_bytes(pl->lanes, &need);
    if (stats && (!pl->active_masks || !pl->workspace || pl->workspace_bytes < need || ((uintptr_t)pl->workspace & 7)))
        return bad("normalized needs active_masks and an 8-byte aligned workspace of gmpe_returns_workspace_bytes(lanes)");
    if (num_partials(pl->lanes) > 0x7fffffffLL) return bad("too many lanes for one launch");
    return GMPE_OK;
}

RetArgs returns_args(const gmpe_returns_plan* pl) {
    RetArgs a;
    a.T = pl->num_steps; a.lanes = pl->lanes; a.stride = pl->stride;
    a.g = (float)pl->gamma;
    a.gl = (float)(pl->gamma * pl->gae_lambda);      // Python: self.gamma * self.gae_lambda in double, then float32 against the arrays
    a.rew = pl->rewards; a.masks = pl->masks; a.bad = pl->bad_masks; a.nv = pl->next_value; a.mu = pl->denorm_mean; a.sd = pl->denorm_std;
    a.am = pl->active_masks; a.vp = pl->value_preds; a.ret = pl->returns;
    a.adv = pl->advantages ? pl->advantages : pl->normalized;
    a.part = pl->normalized ? static_cast<Stat*>(pl->workspace) : nullptr;
    return a;
}

// the recurrence (or the advantages alone) of a plan: one launch
int launch_returns(const gmpe_returns_plan* pl, const RetArgs& a, hipStream_t st) {
    const bool gae = pl->flags & GMPE_RETURNS_GAE, proper = pl->flags & GMPE_RETURNS_PROPER_TIME_LIMITS, only = pl->flags & GMPE_RETURNS_ADVANTAGES_ONLY;
    const dim3 grid((unsigned)num_partials(pl->lanes)), block(RET_BLOCK);
    const bool dn = pl->denorm_mean != nullptr;
    if (only) {
        if (dn) hipLaunchKernelGGL((k_advantages<true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_advantages<false>), grid, block, 0, st, a);
    } else {
        switch ((gae ? 4 : 0) | (proper ? 2 : 0) | (dn ? 1 : 0)) {
        case 0: hipLaunchKernelGGL((k_returns<false, false, false>), grid, block, 0, st, a); break;
        case 1: hipLaunchKernelGGL((k_returns<false, false, true>), grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL((k_returns<false, true, false>), grid, block, 0, st, a); break;
        case 3: hipLaunchKernelGGL((k_returns<false, true, true>), grid, block, 0, st, a); break;
        case 4: hipLaunchKernelGGL((k_returns<true, false, false>), grid, block, 0, st, a); break;
        case 5: hipLaunchKernelGGL((k_returns<true, false, true>), grid, block, 0, st, a); break;
        case 6: hipLaunchKernelGGL((k_returns<true, true, false>), grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL((k_returns<true, true, true>), grid, block, 0, st, a); break;
        }
    }
    GMPE_HIP_CHECK(hipGetLastError());
    return GMPE_OK;
}

// A checked plan, for both entry points: the recurrence (or the advantages alone) unless the shards' statistics are given (`all`), the statistics when
// they are wanted, the normalisation unless the statistics are all that is asked for (`local`). (null, 0, null) is the unsharded call: 3 launches with
// statistics, 1 without; LOCAL 2, APPLY 2.
int run_plan(int device, const gmpe_returns_plan* pl, void* stream, const double* all, int world, double* local) {
    const int64_t nparts = num_partials(pl->lanes);
    GMPE_HIP_CHECK(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const RetArgs a = returns_args(pl);
    if (!all)
        if (int rc = launch_returns(pl, a, st)) return rc;
    if (!pl->normalized) return GMPE_OK;
    float* stats = reinterpret_cast<float*>(static_cast<Stat*>(pl->workspace) + nparts);
    hipLaunchKernelGGL(k_adv_stats, dim3(1), dim3(STAT_BLOCK), 0, st, a.part, nparts, all, world, local, stats);
    GMPE_HIP_CHECK(hipGetLastError());
    if (local) return GMPE_OK;
    hipLaunchKernelGGL(k_adv_normalize, dim3((unsigned)((pl->lanes + NORM_BLOCK - 1) / NORM_BLOCK)), dim3(NORM_BLOCK), 0, st, a.adv, pl->normalized, stats,
                       a.T, pl->lanes, pl->stride);
    GMPE_HIP_CHECK(hipGetLastError());
    return GMPE_OK;
}

}  // namespace

extern "C" {

int gmpe_returns_workspace_bytes(int64_t lanes, size_t* bytes_out) {
    if (!bytes_out || lanes < 1) return fail(GMPE_ERR_INVALID_ARG, "gmpe_returns_workspace_bytes: bad arguments");
    *bytes_out = (size_t)num_partials(lanes) * sizeof(Stat) + 2 * sizeof(float);
    return GMPE_OK;
}

int gmpe_compute_returns(int device, const gmpe_returns_plan* pl, void* stream) {
    if (!pl) return fail(GMPE_ERR_INVALID_ARG, "gmpe_compute_returns: null plan");
    if (int rc = check_returns_plan("gmpe_compute_returns", pl, pl->normalized != nullptr)) return rc;
    return run_plan(device, pl, stream, nullptr, 0, nullptr);
}

int gmpe_compute_returns_shard(int device, const gmpe_returns_shard_plan* sp, void* stream) {
    const char* name = "gmpe_compute_returns_shard";
    if (!sp) return fail(GMPE_ERR_INVALID_ARG, "gmpe_compute_returns_shard: null plan");
    if (int rc = gmpe::check_shard_args(name, sp->phase, sp->world, sp->local, sp->all)) return rc;
    if (!sp->base.normalized) return fail(GMPE_ERR_INVALID_ARG, "gmpe_compute_returns_shard: normalized is required");
    if (int rc = check_returns_plan(name, &sp->base, true)) return rc;
    const bool local = sp->phase == GMPE_SHARD_LOCAL;
    return run_plan(device, &sp->base, stream, local ? nullptr : sp->all, (int)sp->world, local ? sp->local : nullptr);
}

int gmpe_available_actions_from_dones(int device, const gmpe_avail_plan* pl, void* stream) {
    if (!pl || !pl->dones || !pl->available_actions) return fail(GMPE_ERR_INVALID_ARG, "gmpe_available_actions_from_dones: null argument");
    if (pl->lanes < 1 || pl->n_actions < 1 || pl->num_positions < 1 || pl->num_positions > 65535 || pl->first < 0 || pl->first >= pl->num_positions ||
        pl->count < 0)
        return fail(GMPE_ERR_INVALID_ARG, "gmpe_available_actions_from_dones: need lanes, n_actions >= 1, 1 <= num_positions <= 65535, 0 <= first < num_positions, count >= 0");
    const int64_t per_pos = pl->lanes * (int64_t)pl->n_actions;
    if (per_pos > 0x7fffffffLL) return fail(GMPE_ERR_INVALID_ARG, "gmpe_available_actions_from_dones: lanes * n_actions must fit 31 bits");
    if (pl->stride_dones < pl->lanes || pl->stride_out < per_pos)
        return fail(GMPE_ERR_INVALID_ARG, "gmpe_available_actions_from_dones: strides smaller than a slot");
    const int steps = pl->count < pl->num_positions ? pl->count : pl->num_positions;   // positions repeat after T steps: each is written once
    if (steps == 0) return GMPE_OK;
    GMPE_HIP_CHECK(hipSetDevice(device));
    hipLaunchKernelGGL(k_stop_actions, dim3((unsigned)((per_pos + AVAIL_BLOCK - 1) / AVAIL_BLOCK), (unsigned)steps), dim3(AVAIL_BLOCK), 0,
                       static_cast<hipStream_t>(stream), pl->dones, pl->available_actions, (uint32_t)per_pos, (uint32_t)pl->n_actions,
                       pl->num_positions, pl->first, pl->stride_dones, pl->stride_out);
    GMPE_HIP_CHECK(hipGetLastError());
    return GMPE_OK;
}

}  // extern "C"
