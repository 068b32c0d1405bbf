// gmpe_host.h — what the host halves of the learner-side files share (internal: not installed, nothing here has external linkage).
//   * every file: the library's error text and the one HIP-check macro;
//   * the two sharded entry points (gmpe_compute_returns_shard, gmpe_ppo_loss_shard): the checks of their phase, world, `local` and `all`;
//   * every file whose kernels take more than the default 48 KiB of dynamic LDS: the once-per-device raise of that limit;
//   * the layer files (gmpe_gru.hip, gmpe_mlp.hip, gmpe_gnn.hip, gmpe_head.hip, gmpe_value.hip): the grid of resident workgroups, what a valid plan pointer and a valid
//     workspace are, the prologue of their *_workspace_bytes entries, the carving of a workspace, and the launch-and-check macro;
//   * the entry points over gmpe_ppo_rows.h (gmpe_ppo_loss, gmpe_ppo_loss_popart, gmpe_act_sample, and gmpe_head.hip's three): the tile geometry the host
//     fills and the row kernels read, and the checks and the float hyper-parameters the two loss entry points have in common.
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

namespace gmpe {

static int fail(const char* fn, const std::string& m) { return report_error(GMPE_ERR_INVALID_ARG, std::string(fn) + ": " + m); }

// A kernel that needs more than the default 48 KiB of dynamic LDS: raise the limit of instantiation `slot` of this file to `bytes`, the largest size
// there is, once per device. The table has internal linkage: every .hip file numbers its own instantiations. A device or a slot outside the table is set
// at every call.
constexpr int LDS_DEVICES = 64, LDS_SLOTS = 4;
static int raise_dynamic_lds_once(const void* fn, int device, int slot, size_t bytes) {
    static std::atomic<bool> raised[LDS_DEVICES][LDS_SLOTS];
    const bool cached = device >= 0 && device < LDS_DEVICES && slot >= 0 && slot < LDS_SLOTS;
    if (cached && raised[device][slot].load()) return GMPE_OK;
    GMPE_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    if (cached) raised[device][slot].store(true);
    return GMPE_OK;
}

// ---- the layer files: gmpe_gru.hip, gmpe_mlp.hip, gmpe_gnn.hip, gmpe_head.hip, gmpe_value.hip

constexpr int MAX_CU = 256, LDS_CU = 160 * 1024;        // the CUs a grid is sized for, and the LDS of one of them in bytes

// The grid of a kernel whose workgroups own tiles blockIdx.x, blockIdx.x + gridDim.x, ...: as many workgroups as the CUs hold at once, by LDS
// (`lds` bytes per workgroup) and at most `cap` per CU; fewer where there are fewer tiles.
static int resident_grid(int64_t tiles, size_t lds, int cap) {
    int per = (int)(LDS_CU / lds);
    per = per < 1 ? 1 : (per > cap ? cap : per);
    const int64_t g = (int64_t)MAX_CU * per;
    return (int)(tiles < g ? tiles : g);
}

// A plan's pointer to float32 or int32 device memory: there if needed, 4-byte aligned whether needed or not.
static int check_ptr(const char* fn, const void* p, const std::string& name, bool need) {
    if (need && !p) return fail(fn, name + " is required");
    if ((uintptr_t)p & 3) return fail(fn, name + " must be 4-byte aligned");
    return GMPE_OK;
}

// ... and a table of them in the order they are complained about, their names behind `prefix` ("layer[1].", "conv[0].")
struct PtrField { const void* ptr; const char* name; bool need; };
template <size_t N>
static int check_ptrs(const char* fn, const PtrField (&fields)[N], const std::string& prefix = std::string()) {
    for (const PtrField& f : fields)
        if (int rc = check_ptr(fn, f.ptr, prefix + f.name, f.need)) return rc;
    return GMPE_OK;
}

// A plan's workspace of at least `total` bytes: there if needed (`required`: the entry point's words for a missing one), checked whenever there.
// `query`: the call that gives `total`, as the complaint names it.
static int check_workspace(const char* fn, const void* workspace, size_t bytes, size_t total, bool need, const char* required, const char* query) {
    if (need && !workspace) return fail(fn, required);
    if (workspace) {
        if ((uintptr_t)workspace & 7) return fail(fn, "workspace must be 8-byte aligned");
        if (bytes < total) return fail(fn, std::string("workspace_bytes is below ") + query + " = " + std::to_string(total));
    }
    return GMPE_OK;
}

// What the three *_workspace_bytes entries check of the two arguments they share. `dims`: the entry point's own finding about the dimensions it is
// built for (empty: none), reported at its place between the two.
static int check_workspace_query(const char* fn, const size_t* bytes_out, const std::string& dims, int want_backward) {
    if (!bytes_out) return fail(fn, "bytes_out is null");
    if (!dims.empty()) return fail(fn, dims);
    if (want_backward != 0 && want_backward != 1) return fail(fn, "want_backward must be 0 or 1");
    return GMPE_OK;
}

// A workspace carved front to back: take() gives the offset of the next `bytes`, total() the size rounded up to 8, at<T>() the place of an offset in
// a plan's workspace (null for a forward-only plan's null workspace).
struct Carver {
    size_t o = 0;
    size_t take(size_t bytes) { const size_t off = o; o += bytes; return off; }
    size_t total() const { return (o + 7) & ~(size_t)7; }
};
template <class T>
static T* at(void* workspace, size_t off) { return workspace ? reinterpret_cast<T*>(static_cast<char*>(workspace) + off) : nullptr; }

}  // namespace gmpe

// One kernel launch and its check: hipLaunchKernelGGL's own arguments, in its order.
#define GMPE_LAUNCH(kernel, grid, block, lds, stream, ...) \
    do { hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__); GMPE_HIP_CHECK(hipGetLastError()); } while (0)

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

}  // namespace gmpe_ppo
