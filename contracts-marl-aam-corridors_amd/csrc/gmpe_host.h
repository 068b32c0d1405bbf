// gmpe_host.h — what the host halves of the learner-side files share (internal: not installed, nothing here has external linkage).
//   * every file: the library's error text and the one HIP-check macro;
//   * the two sharded entry points (gmpe_compute_returns_shard, gmpe_ppo_loss_shard): the checks of their phase, world, `local` and `all`;
//   * the three entry points over gmpe_ppo_rows.h (gmpe_ppo_loss, gmpe_ppo_loss_popart, gmpe_act_sample): the tile geometry the host fills and the row
//     kernels read, the checks and the float hyper-parameters the two loss entry points have in common, and the once-per-device raise of the dynamic LDS limit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <string>

#include "../../include/gmpe.h"

namespace gmpe {
int report_error(int code, const std::string& m);   // gmpe_step.hip: the library's gmpe_last_error text

// What the two sharded entry points (`name`: gmpe_compute_returns_shard, gmpe_ppo_loss_shard) check of their own fields, before their base plan's checks.
static int check_shard_args(const char* name, int phase, int world, const double* local, const double* all) {
    const auto bad = [&](const char* m) { return report_error(GMPE_ERR_INVALID_ARG, std::string(name) + ": " + m); };
    if (phase != GMPE_SHARD_LOCAL && phase != GMPE_SHARD_APPLY) return bad("phase must be GMPE_SHARD_LOCAL or GMPE_SHARD_APPLY");
    if (world < 1 || world > GMPE_SHARD_MAX_WORLD) return bad("world must be in 1 .. 4096");
    const double* stat_ptr = phase == GMPE_SHARD_LOCAL ? local : all;
    if (!stat_ptr || ((uintptr_t)stat_ptr & 7)) return bad("LOCAL needs `local`, APPLY needs `all`, f64 device memory, 8-byte aligned");
    return GMPE_OK;
}
}

#define GMPE_HIP_CHECK(x) \
    do { hipError_t e_ = (x); if (e_ != hipSuccess) return gmpe::report_error(GMPE_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

namespace gmpe_ppo {

constexpr int TILE = 256;         // rows per workgroup = lanes per workgroup: one lane per row

// Where a row kernel's tiles lie: B rows of K floats; a tile's rows stand in LDS at stride S.
struct Geom {
    int64_t B;
    int K, S;                      // S: LDS row stride in dwords, odd, so the 32 lanes of a ds_read_b32 group (stride S) hit 32 distinct banks
    uint32_t magic;                // floor(2^32 / K) + 1: f / K == umulhi(f, magic) for f < 2^16 (a tile holds at most TILE * 64 floats)
};

static inline int64_t num_tiles(int64_t rows) { return (rows + TILE - 1) / TILE; }

static inline Geom geometry(int64_t rows, int n_actions) {
    Geom g;
    g.B = rows; g.K = n_actions; g.S = n_actions | 1;
    g.magic = (uint32_t)((1ULL << 32) / (uint64_t)(n_actions > 1 ? n_actions : 2)) + 1u;
    return g;
}

// The checks gmpe_ppo_loss and gmpe_ppo_loss_popart make alike, in the order both make them. `dims` and `missing` are the entry point's own findings about
// its further dimensions and its required pointers (null: none), reported at their place in that order. No string is formed unless a check fails.
template <class Plan>
static int check_loss_plan(const char* name, const Plan* pl, const char* dims, const char* missing) {
    const auto bad = [&](const std::string& m) { return gmpe::report_error(GMPE_ERR_INVALID_ARG, std::string(name) + ": " + m); };
    if (pl->rows < 1) return bad("need rows >= 1");
    if (pl->n_actions < 1 || pl->n_actions > GMPE_PPO_MAX_ACTIONS) return bad("n_actions must be in 1 .. " + std::to_string(GMPE_PPO_MAX_ACTIONS));
    if (dims) return bad(dims);
    if (pl->actions_int64 != 0 && pl->actions_int64 != 1) return bad("actions_int64 must be 0 or 1");
    if (missing) return bad(missing);
    if (!(pl->clip_param >= 0.0) || !(pl->huber_delta >= 0.0) || !(pl->beta >= 0.0 && pl->beta <= 1.0) || !(pl->epsilon > 0.0) || pl->entropy_coef != pl->entropy_coef)
        return bad("need clip_param >= 0, huber_delta >= 0, 0 <= beta <= 1, epsilon > 0 and a number for entropy_coef");
    return GMPE_OK;
}

// The plan's doubles as the float32 numbers the kernels compute with, into the fields LossArgs and PopArgs name alike.
// A Python float meets a float32 tensor as float32(value): 1.0 - clip_param, 1.0 - beta and huber_delta / 2 are formed in double first.
template <class Plan, class Args>
static void hyper_parameters(const Plan* pl, Args& a) {
    a.pol.lo = (float)(1.0 - pl->clip_param); a.pol.hi = (float)(1.0 + pl->clip_param); a.clip = (float)pl->clip_param;
    a.delta = (float)pl->huber_delta; a.half_delta = (float)(pl->huber_delta / 2.0); a.pol.ent_coef = (float)pl->entropy_coef;
    a.wbeta = (float)pl->beta; a.w1beta = (float)(1.0 - pl->beta); a.eps = (float)pl->epsilon;
}

// A row kernel whose tile needs more than the default 48 KiB of dynamic LDS: raise the limit of instantiation `slot` of this file to `bytes`, the largest
// size there is, once per device. The table has internal linkage: every .hip file numbers its own instantiations. A device outside the table is set at
// every call.
constexpr int LDS_DEVICES = 64, LDS_SLOTS = 4;
static int raise_dynamic_lds_once(const void* fn, int device, int slot, size_t bytes) {
    static std::atomic<bool> raised[LDS_DEVICES][LDS_SLOTS];
    const bool cached = device >= 0 && device < LDS_DEVICES;
    if (cached && raised[device][slot].load()) return GMPE_OK;
    GMPE_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    if (cached) raised[device][slot].store(true);
    return GMPE_OK;
}

}  // namespace gmpe_ppo
