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

#include "gmpe_act_rows.h"       // gmpe_device.h, gmpe_host.h (include/gmpe.h, the error text, GMPE_HIP_CHECK), gmpe_ppo_rows.h; the row's routine, shared with gmpe_head.hip

#pragma clang fp contract(off)

namespace {

using namespace gmpe_ppo;         // gmpe_ppo_rows.h: TILE, the tile machinery and the masked categorical

// One lane per row; the tile's available_actions (when given), then its logits, pass through the same LDS rows.
template <bool VEC>
__global__ __launch_bounds__(TILE) void k_act_rows(ActArgs p) {
    extern __shared__ __attribute__((aligned(16))) float sh[];
    const Tile t = tile_of(p.g, sh);
    const uint64_t avail = tile_in<VEC>(p.g, t, p.avail, p.logits, sh, act_avail0(p, t));
    if (!t.live) return;
    act_row(p, t.r, t.row, avail);
}

// after the rows of this call have read the counter (same stream): the next replay of a captured graph draws fresh numbers
__global__ void k_act_advance(uint64_t* draw_dev, uint64_t inc) { *draw_dev += inc; }

}  // namespace

namespace gmpe {

int check_act_plan(const char* fn, const gmpe_act_plan* pl, bool given_logits) {
    if (!pl) return fail(fn, "null plan");
    if (pl->rows < 1) return fail(fn, "need rows >= 1");
    if (pl->n_actions < 1 || pl->n_actions > GMPE_PPO_MAX_ACTIONS) return fail(fn, "n_actions must be in 1 .. " + std::to_string(GMPE_PPO_MAX_ACTIONS));
    if (pl->num_agents < 1) return fail(fn, "need num_agents >= 1");
    if (pl->stop_action < 0 || pl->stop_action >= pl->n_actions) return fail(fn, "stop_action must be in 0 .. n_actions - 1");
    if (pl->deterministic != 0 && pl->deterministic != 1) return fail(fn, "deterministic must be 0 or 1");
    if (pl->reserved != 0) return fail(fn, "reserved must be 0");
    if (pl->available_actions && pl->dones_prev)
        return fail(fn, "available_actions and dones_prev are two sources of the availability: give at most one");
    if (given_logits && !pl->logits) return fail(fn, "logits is required");
    if (!given_logits && pl->logits) return fail(fn, "act_plan->logits must be NULL: the logits are formed from head_plan->features");
    if (!pl->action_idx) return fail(fn, "action_idx is required");
    if (!pl->log_probs) return fail(fn, "log_probs is required");
    const uintptr_t a4 = (uintptr_t)pl->logits | (uintptr_t)pl->available_actions | (uintptr_t)pl->action_idx | (uintptr_t)pl->log_probs | (uintptr_t)pl->actions_f32;
    if ((a4 & 3) || (((uintptr_t)pl->actions_i64 | (uintptr_t)pl->draw_dev) & 7))
        return fail(fn, "f32 / int32 arrays must be 4-byte aligned, actions_i64 and draw_dev 8-byte aligned");
    if (gmpe_ppo::num_tiles(pl->rows) > 0x7fffffffLL) return fail(fn, "too many rows for one launch");
    return GMPE_OK;
}

int act_advance(uint64_t* draw_dev, uint64_t inc, hipStream_t stream) {
    GMPE_LAUNCH(k_act_advance, dim3(1), dim3(1), 0, stream, draw_dev, inc);
    return GMPE_OK;
}

}  // namespace gmpe

extern "C" {

int gmpe_act_sample(int device, const gmpe_act_plan* pl, void* stream) {
    if (int rc = gmpe::check_act_plan("gmpe_act_sample", pl, true)) return rc;
    GMPE_HIP_CHECK(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const ActArgs a = act_args(pl);
    const bool vec = !(((uintptr_t)pl->logits | (uintptr_t)pl->available_actions) & 15);        // tiles start at multiples of 1 KiB
    const size_t lds = (size_t)TILE * a.g.S * sizeof(float);
    void (*fn)(ActArgs) = vec ? k_act_rows<true> : k_act_rows<false>;
    if (lds > 48 * 1024)                                                      // K = 64 only
        if (int rc = gmpe::raise_dynamic_lds_once(reinterpret_cast<const void*>(fn), device, vec, TILE * (GMPE_PPO_MAX_ACTIONS | 1) * sizeof(float)))
            return rc;
    GMPE_LAUNCH(fn, dim3((unsigned)num_tiles(pl->rows)), dim3(TILE), lds, st, a);
    if (pl->draw_dev && pl->draw_inc) return gmpe::act_advance(pl->draw_dev, pl->draw_inc, st);   // adding zero changes nothing: no launch
    return GMPE_OK;
}

}  // extern "C"
