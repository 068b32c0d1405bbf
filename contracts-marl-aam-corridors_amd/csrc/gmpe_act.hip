// gmpe_act.hip — the rollout half of the discrete action head (include/gmpe.h gmpe_act_sample): the masked categorical of the policy's logits, one action
// per row by inverse CDF (or the mode), and that action's log-prob, in one launch. Handle-less, like gmpe_ppo_loss.
//
// What is restated: ACTLayer.forward (onpolicy/algorithms/utils/act.py:107-113) = Categorical.forward (distributions.py:84-91: logits at
// finfo(float32).min where available_actions == 0, FixedCategorical(logits=x)), then sample() or mode() (:15-16, 27-28), then log_probs (:18-25); and
// what the runner does with the result (graph_mpe_runner.py:299-320, 356-377): the int action the env takes, the float32 / int64 action the buffer keeps.
//
// The distribution of a row is policy_row's: this kernel calls the helpers policy_row is made of (gmpe_ppo_rows.h masked_max, normalise_row, prob), so
// the log-prob l[a] written here has the bits gmpe_ppo_loss recomputes for the same logits, availability and action: the first minibatch of an unchanged
// policy has importance weights of exactly 1. The tile machinery is that header's too.
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

#include <string>

#include "gmpe_device.h"
#include "gmpe_host.h"          // include/gmpe.h, the error text, GMPE_HIP_CHECK
#include "gmpe_ppo_rows.h"

#pragma clang fp contract(off)

namespace {

using namespace gmpe_ppo;         // gmpe_ppo_rows.h: TILE, the tile machinery and the masked categorical

struct ActArgs {
    Geom g;
    int A, stop, det;
    uint32_t env_base;
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
    const int K = p.g.K;
    const Tile t = tile_of(p.g, sh);
    const int64_t r = t.r;
    float* row = t.row;
    const uint64_t all = K == 64 ? ~0ull : (1ull << K) - 1ull;

    uint64_t avail = all;
    if (!p.avail && p.dones && t.live && p.dones[r]) avail = 1ull << p.stop;         // collect_with_mask: a done agent may only stop
    avail = tile_in<VEC>(p.g, t, p.avail, p.logits, sh, avail);
    if (!t.live) return;

    // ---- the masked categorical, as policy_row forms it; the mode is taken while the row still holds the logits (rounding x - lse can make ties)
    const float m = masked_max(row, K, avail);
    const uint64_t set = avail ? avail : all;                                       // nothing available: the uniform row over all K
    int mode = __builtin_ctzll(set);
    for (int j = K - 1; j >= 0; --j)
        if ((set >> j & 1) && masked_logit(row, avail, j) == m) mode = j;           // the first index of the largest masked logit
    float ml, s2;
    normalise_row(row, K, avail, m, &ml, &s2);
    int a = mode;
    if (!p.det) {
        const int64_t env = r / p.A;
        const uint64_t agent = (uint64_t)(r - env * p.A);
        const uint64_t d = p.draw + (p.draw_dev ? *p.draw_dev : 0ull);
        const double u = gmpe::philox_uniform(p.seed, p.env_base + (uint32_t)env, 0x8000000000000000ull | (d * (uint64_t)p.A + agent));
        float c = 0.0f;
        for (int j = 0; j < K; ++j) {
            if (!(set >> j & 1)) continue;
            c = __fadd_rn(c, prob(row[j], ml, s2));
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
    const int64_t nt = num_tiles(pl->rows);
    if (nt > 0x7fffffffLL) return fail(GMPE_ERR_INVALID_ARG, "gmpe_act_sample: too many rows for one launch");
    GMPE_HIP_CHECK(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    ActArgs a;
    a.g = geometry(pl->rows, pl->n_actions);
    a.A = pl->num_agents; a.stop = pl->stop_action; a.det = pl->deterministic;
    a.env_base = (uint32_t)pl->env_id_base;
    a.seed = pl->seed; a.draw = pl->draw; a.draw_dev = pl->draw_dev;
    a.logits = pl->logits; a.avail = pl->available_actions; a.dones = pl->dones_prev;
    a.idx = pl->action_idx; a.lp = pl->log_probs; a.af = pl->actions_f32; a.ai = pl->actions_i64;
    const bool vec = !(((uintptr_t)pl->logits | (uintptr_t)pl->available_actions) & 15);        // tiles start at multiples of 1 KiB
    const size_t lds = (size_t)TILE * a.g.S * sizeof(float);
    void (*fn)(ActArgs) = vec ? k_act_rows<true> : k_act_rows<false>;
    if (lds > 48 * 1024)                                                      // K = 64 only
        if (int rc = gmpe::raise_dynamic_lds_once(reinterpret_cast<const void*>(fn), device, vec, TILE * (GMPE_PPO_MAX_ACTIONS | 1) * sizeof(float)))
            return rc;
    hipLaunchKernelGGL(fn, dim3((unsigned)nt), dim3(TILE), lds, st, a);
    GMPE_HIP_CHECK(hipGetLastError());
    if (pl->draw_dev) {
        hipLaunchKernelGGL(k_act_advance, dim3(1), dim3(1), 0, st, pl->draw_dev, pl->draw_inc);
        GMPE_HIP_CHECK(hipGetLastError());
    }
    return GMPE_OK;
}

}  // extern "C"
