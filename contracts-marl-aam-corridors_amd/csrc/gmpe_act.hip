// gmpe_act.hip — the rollout half of the discrete action head (include/gmpe.h gmpe_act_sample): the masked categorical of the policy's logits, one action
// per row by inverse CDF (or the mode), and that action's log-prob, in one launch. Handle-less, like gmpe_ppo_loss.
//
// What is restated: ACTLayer.forward (onpolicy/algorithms/utils/act.py:107-113) = Categorical.forward (distributions.py:84-91: logits at
// finfo(float32).min where available_actions == 0, FixedCategorical(logits=x)), then sample() or mode() (:15-16, 27-28), then log_probs (:18-25); and
// what the runner does with the result (graph_mpe_runner.py:299-320, 356-377): the int action the env takes, the float32 / int64 action the buffer keeps.
//
// The distribution of a row is policy_row's (gmpe_ppo_rows.h), restated here with the same intrinsics in the same order — max, lse, l = x - lse, ml,
// p_j = exp(l_j - ml) / s2 — so the log-prob l[a] written here has the bits gmpe_ppo_loss recomputes for the same logits, availability and action: the
// first minibatch of an unchanged policy has importance weights of exactly 1. The header itself is included for its tile machinery and left as it is.
//
// Sampling: one draw u per row from the project's Philox stream (gmpe_device.h philox_uniform), keyed by the row's ENV and agent, not by where the row
// lies in the batch: u = philox_uniform(seed, env_id_base + r / A, 2^63 | (draw * A + r % A)). The top bit keeps the action stream apart from the env's
// own draw counter, which counts up from 0. c_j = the running float32 sum of p_j over the available j in index order; the action is the first available
// j with (double)c_j > u, or the mode when u lies above the rounded total. An unavailable action is never returned. A row with no available action
// follows policy_row's arithmetic — the reference's uniform row over all K actions, log-prob 0 — and is sampled over all K.
// The mode is the first index of the largest masked logit.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include <atomic>
#include <string>

#include "../../include/gmpe.h"
#include "gmpe_device.h"
#include "gmpe_ppo_rows.h"

#pragma clang fp contract(off)

namespace gmpe {
int report_error(int code, const std::string& m);   // gmpe_step.hip: the library's gmpe_last_error text
}

namespace {

using namespace gmpe_ppo;         // gmpe_ppo_rows.h: TILE, FMIN, tile_copy, avail_bits

struct ActArgs {
    int64_t B;
    int K, S, A, stop, det;        // S: LDS row stride in dwords, odd (gmpe_ppo_loss.hip LossArgs)
    uint32_t magic, env_base;
    uint64_t seed, draw;
    const uint64_t* draw_dev;
    const float *logits, *avail;
    const uint8_t* dones;
    int32_t* idx;
    float *lp, *af;
    int64_t* ai;
};

// One lane per row; the tile's available_actions (when given), then its logits, pass through the same LDS rows.
template <bool VEC>
__global__ __launch_bounds__(TILE) void k_act_rows(ActArgs p) {
    extern __shared__ __attribute__((aligned(16))) float sh[];
    const int K = p.K, S = p.S;
    const int64_t row0 = (int64_t)blockIdx.x * TILE, r = row0 + threadIdx.x;
    const int rows = p.B - row0 < TILE ? (int)(p.B - row0) : TILE, n = rows * K;
    const bool live = (int)threadIdx.x < rows;
    float* row = sh + threadIdx.x * S;
    const int64_t g0 = row0 * K;
    const uint64_t all = K == 64 ? ~0ull : (1ull << K) - 1ull;

    uint64_t avail = all;
    if (p.avail) {
        tile_copy<VEC, true>(const_cast<float*>(p.avail) + g0, sh, n, K, S, p.magic);
        __syncthreads();
        if (live) avail = avail_bits(row, K);                                       // x[available_actions == 0] = finfo.min
        __syncthreads();
    } else if (p.dones && live && p.dones[r]) {
        avail = 1ull << p.stop;                                                     // collect_with_mask: a done agent may only stop
    }
    tile_copy<VEC, true>(const_cast<float*>(p.logits) + g0, sh, n, K, S, p.magic);
    __syncthreads();
    if (!live) return;

    // ---- the masked categorical, as policy_row forms it
    float m = -INFINITY;
    for (int j = 0; j < K; ++j) m = fmaxf(m, (avail >> j & 1) ? row[j] : FMIN);
    const uint64_t set = avail ? avail : all;                                       // nothing available: the uniform row over all K
    int mode = __builtin_ctzll(set);
    for (int j = K - 1; j >= 0; --j)
        if ((set >> j & 1) && ((avail >> j & 1) ? row[j] : FMIN) == m) mode = j;    // the first index of the largest masked logit
    float s = 0.0f;
    for (int j = 0; j < K; ++j) s = __fadd_rn(s, expf(__fsub_rn((avail >> j & 1) ? row[j] : FMIN, m)));
    const float lse = __fadd_rn(logf(s), m), ml = __fsub_rn(m, lse);
    float s2 = 0.0f;
    for (int j = 0; j < K; ++j) {                                                   // the row now holds l = x - logsumexp(x)
        const float l = __fsub_rn((avail >> j & 1) ? row[j] : FMIN, lse);
        row[j] = l;
        s2 = __fadd_rn(s2, expf(__fsub_rn(l, ml)));
    }
    int a = mode;
    if (!p.det) {
        const int64_t env = r / p.A;
        const uint64_t agent = (uint64_t)(r - env * p.A);
        const uint64_t d = p.draw + (p.draw_dev ? *p.draw_dev : 0ull);
        const double u = gmpe::philox_uniform(p.seed, p.env_base + (uint32_t)env, 0x8000000000000000ull | (d * (uint64_t)p.A + agent));
        float c = 0.0f;
        for (int j = 0; j < K; ++j) {
            if (!(set >> j & 1)) continue;
            c = __fadd_rn(c, __fdiv_rn(expf(__fsub_rn(row[j], ml)), s2));
            if ((double)c > u) { a = j; break; }
        }
    }
    p.idx[r] = a;
    p.lp[r] = row[a];
    if (p.af) p.af[r] = (float)a;
    if (p.ai) p.ai[r] = (int64_t)a;
}

// after the rows of this call have read the counter (same stream): the next replay of a captured graph draws fresh numbers
__global__ void k_act_advance(uint64_t* draw_dev, uint64_t inc) { *draw_dev += inc; }

int fail(int code, const std::string& m) { return gmpe::report_error(code, m); }

}  // namespace

#define ACHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(GMPE_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

extern "C" {

int gmpe_act_sample(int device, const gmpe_act_plan* pl, void* stream) {
    if (!pl) return fail(GMPE_ERR_INVALID_ARG, "gmpe_act_sample: null plan");
    if (pl->rows < 1) return fail(GMPE_ERR_INVALID_ARG, "gmpe_act_sample: need rows >= 1");
    if (pl->n_actions < 1 || pl->n_actions > GMPE_PPO_MAX_ACTIONS)
        return fail(GMPE_ERR_INVALID_ARG, "gmpe_act_sample: n_actions must be in 1 .. " + std::to_string(GMPE_PPO_MAX_ACTIONS));
    if (pl->num_agents < 1) return fail(GMPE_ERR_INVALID_ARG, "gmpe_act_sample: need num_agents >= 1");
    if (pl->stop_action < 0 || pl->stop_action >= pl->n_actions) return fail(GMPE_ERR_INVALID_ARG, "gmpe_act_sample: stop_action must be in 0 .. n_actions - 1");
    if (pl->deterministic != 0 && pl->deterministic != 1) return fail(GMPE_ERR_INVALID_ARG, "gmpe_act_sample: deterministic must be 0 or 1");
    if (pl->reserved != 0) return fail(GMPE_ERR_INVALID_ARG, "gmpe_act_sample: reserved must be 0");
    if (pl->available_actions && pl->dones_prev)
        return fail(GMPE_ERR_INVALID_ARG, "gmpe_act_sample: available_actions and dones_prev are two sources of the availability: give at most one");
    if (!pl->logits) return fail(GMPE_ERR_INVALID_ARG, "gmpe_act_sample: logits is required");
    if (!pl->action_idx) return fail(GMPE_ERR_INVALID_ARG, "gmpe_act_sample: action_idx is required");
    if (!pl->log_probs) return fail(GMPE_ERR_INVALID_ARG, "gmpe_act_sample: log_probs is required");
    const uintptr_t a4 = (uintptr_t)pl->logits | (uintptr_t)pl->available_actions | (uintptr_t)pl->action_idx | (uintptr_t)pl->log_probs | (uintptr_t)pl->actions_f32;
    if ((a4 & 3) || (((uintptr_t)pl->actions_i64 | (uintptr_t)pl->draw_dev) & 7))
        return fail(GMPE_ERR_INVALID_ARG, "gmpe_act_sample: f32 / int32 arrays must be 4-byte aligned, actions_i64 and draw_dev 8-byte aligned");
    const int64_t nt = (pl->rows + TILE - 1) / TILE;
    if (nt > 0x7fffffffLL) return fail(GMPE_ERR_INVALID_ARG, "gmpe_act_sample: too many rows for one launch");
    ACHK(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    ActArgs a;
    a.B = pl->rows; a.K = pl->n_actions; a.S = pl->n_actions | 1; a.A = pl->num_agents; a.stop = pl->stop_action; a.det = pl->deterministic;
    a.magic = (uint32_t)(0x100000000ULL / (uint64_t)(pl->n_actions > 1 ? pl->n_actions : 2)) + 1u;
    a.env_base = (uint32_t)pl->env_id_base;
    a.seed = pl->seed; a.draw = pl->draw; a.draw_dev = pl->draw_dev;
    a.logits = pl->logits; a.avail = pl->available_actions; a.dones = pl->dones_prev;
    a.idx = pl->action_idx; a.lp = pl->log_probs; a.af = pl->actions_f32; a.ai = pl->actions_i64;
    const bool vec = !(((uintptr_t)pl->logits | (uintptr_t)pl->available_actions) & 15);        // tiles start at multiples of 1 KiB
    const size_t lds = (size_t)TILE * a.S * sizeof(float);
    void (*fn)(ActArgs) = vec ? k_act_rows<true> : k_act_rows<false>;
    if (lds > 48 * 1024) {                                                    // K = 64 only; once per device and instantiation, at the largest size there is
        static std::atomic<bool> raised[64][2];
        if (device < 0 || device >= 64 || !raised[device][vec].load()) {
            ACHK(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)(TILE * (GMPE_PPO_MAX_ACTIONS | 1) * sizeof(float))));
            if (device >= 0 && device < 64) raised[device][vec].store(true);
        }
    }
    hipLaunchKernelGGL(fn, dim3((unsigned)nt), dim3(TILE), lds, st, a);
    ACHK(hipGetLastError());
    if (pl->draw_dev) {
        hipLaunchKernelGGL(k_act_advance, dim3(1), dim3(1), 0, st, pl->draw_dev, pl->draw_inc);
        ACHK(hipGetLastError());
    }
    return GMPE_OK;
}

}  // extern "C"
