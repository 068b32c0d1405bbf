// gmpe_act_rows.h — what the two rollout entry points over a policy head share (internal): gmpe_act_sample (gmpe_act.hip: the logits are given) and
// gmpe_act_head (gmpe_head.hip: the logits are formed in the launch from the actor features). One text for the row's arithmetic — the masked categorical,
// the mode, the Philox draw, the inverse CDF, the four stores — so the two cannot drift apart; and the host's checks and argument binding of a gmpe_act_plan.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gmpe_device.h"
#include "gmpe_host.h"
#include "gmpe_ppo_rows.h"

#pragma clang fp contract(off)

namespace gmpe_ppo {

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

// what a row may take before its available_actions (when given) are read: everything, or only the stop action for a done agent (collect_with_mask)
__device__ __forceinline__ uint64_t act_avail0(const ActArgs& p, const Tile& t) {
    const uint64_t all = p.g.K == 64 ? ~0ull : (1ull << p.g.K) - 1ull;
    if (!p.avail && p.dones && t.live && p.dones[t.r]) return 1ull << p.stop;
    return all;
}

// Row r of a live lane: `row` holds its K logits in LDS (and its normalised logits on return), avail its availability bits.
__device__ __forceinline__ void act_row(const ActArgs& p, int64_t r, float* row, uint64_t avail) {
    const int K = p.g.K;
    const uint64_t all = K == 64 ? ~0ull : (1ull << K) - 1ull;
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

// the kernel arguments of a checked plan
static inline ActArgs act_args(const gmpe_act_plan* pl) {
    ActArgs a;
    a.g = geometry(pl->rows, pl->n_actions);
    a.A = pl->num_agents; a.stop = pl->stop_action; a.det = pl->deterministic;
    a.env_base = (uint32_t)pl->env_id_base;
    a.seed = pl->seed; a.draw = pl->draw; a.draw_dev = pl->draw_dev;
    a.logits = pl->logits; a.avail = pl->available_actions; a.dones = pl->dones_prev;
    a.idx = pl->action_idx; a.lp = pl->log_probs; a.af = pl->actions_f32; a.ai = pl->actions_i64;
    return a;
}

}  // namespace gmpe_ppo

namespace gmpe {
// gmpe_act.hip. Everything the host can see of a gmpe_act_plan, complained about in the name `fn`; given_logits: the plan's logits are required (gmpe_act_sample)
// or must be NULL (gmpe_act_head).
int check_act_plan(const char* fn, const gmpe_act_plan* pl, bool given_logits);
// ... and the one-thread launch behind the rows of a call with draw_dev: *draw_dev += inc on `stream`
int act_advance(uint64_t* draw_dev, uint64_t inc, hipStream_t stream);
}
