// gmpe_optim_table.h — what gmpe_optim.hip (gmpe_optim_step) and gmpe_optim_shard.hip (gmpe_optim_step_shard) share (internal: not installed): the table
// of tensors that travels as a kernel argument, the search of an element's tensor, the workgroup sum, and the host half that checks a plan, cuts it into
// launch groups and launches k_opt_step. The host functions are defined once, in gmpe_optim.hip.
#pragma once
#include <math.h>

#include <vector>

#include "gmpe_host.h"

namespace gmpe_opt {

constexpr int BLOCK = 256, CHUNK = GMPE_OPT_CHUNK, PER_THREAD = CHUNK / BLOCK, MAXT = GMPE_OPT_MAX_TENSORS, MAXH = GMPE_OPT_MAX_HYPERS;
constexpr uint32_t GROUP_LIMIT = 0x7fffffffu - (uint32_t)CHUNK;     // a group's elements: every chunk's last index stays below 2^31

struct Desc {
    float* p; float* g; float* m; float* v;
    uint32_t start;                // the tensor's first element in the group's concatenation
    uint16_t flags, hyper;         // GMPE_OPT_T_*; index into Table::h
};
static_assert(sizeof(Desc) == 40, "a descriptor is 40 bytes");

struct Hyper { float wd, w1, b2, w2, a, s2, eps; };
static_assert(sizeof(Hyper) == GMPE_OPT_HYPER_FLOATS * sizeof(float), "a schedule slot is a Hyper: wd, w1, b2, w2, a, s2, eps");

struct Table {
    Desc d[MAXT];
    Hyper h[MAXH];
    uint32_t total;                // the group's elements
    int32_t n;                     // its tensors
};
static_assert(sizeof(Table) <= 3072, "the table and the other arguments stay under the 4 KB of kernel arguments");

// the tensor that holds element e < total: the last i with d[i].start <= e (the starts ascend strictly: empty tensors are not in the table)
__device__ __forceinline__ int find_tensor(const Table& tb, uint32_t e) {
    int lo = 0, hi = tb.n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tb.d[mid].start <= e) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// the 256 sums of a workgroup added pairwise by halving; every thread returns the total
__device__ __forceinline__ double block_sum(double s, double* red) {
    const int tid = threadIdx.x;
    red[tid] = s;
    __syncthreads();
    for (int w = BLOCK / 2; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    const double tot = red[0];
    __syncthreads();
    return tot;
}

struct Layout {
    std::vector<Table> groups;     // at least one: a table without elements still writes `out`
    std::vector<int64_t> chunks;   // per group
    int64_t n_chunks = 0;
    int64_t elems = 0;             // the elements of all groups
    std::vector<int> slot_hyper;   // MAXH per group: the plan's hyper index in each of the group's slots, -1 for a slot not in use
    size_t total = 0;              // workspace bytes
};

// How much of a plan a caller is about to use, and so how much of it is checked and filled into the groups' tables.
enum Depth {
    GEOMETRY,                      // counts, numel, flags, hyper indices: gmpe_optim_workspace_bytes, gmpe_optim_shard_elems
    GRADS,                         // ... and the `grad` pointers: GMPE_SHARD_LOCAL, which reads nothing else
    STEP,                          // everything gmpe_optim_step checks, the workspace included
};

// The checks of `depth` in gmpe_optim_step's order, complaints under the name `fn`, then the launch groups of the plan.
int prepare(const char* fn, const gmpe_optim_plan* pl, Depth depth, Layout& y);
// k_opt_step over every group of a plan prepared with STEP: part[] holds the chunks' sums of all groups (a table without elements: one launch that
// writes `out`).
int launch_steps(const gmpe_optim_plan* pl, const Layout& y, hipStream_t st);
// The float32 set of one param_group at step count t: the ONE place the doubles are rounded — layout() fills the kernel-argument table with it and
// gmpe_optim_schedule_fill the rows of a schedule, so a scheduled step's bits are gmpe_optim_step's by construction.
Hyper make_hyper(const gmpe_optim_hyper& h, int64_t t);
// the values of the plan's hyper-parameter sets: what make_hyper may be given
int check_hypers(const char* fn, const gmpe_optim_plan* pl);
// every group's k_opt_norm into the plan's workspace, the chunks of all groups numbered in group order
int launch_norms(const gmpe_optim_plan* pl, const Layout& y, hipStream_t st);

struct StepArgs {
    const double* part;            // the chunks' sums of ALL groups
    int32_t n_parts;
    int32_t clip, step, first;     // plan flags; first: this launch's workgroup 0 writes out
    double max_norm;
    double* out;
    float* norm_f32;
    // SCHED only (gmpe_optim_step_scheduled): the group's Hyper slots come from row *counter of the schedule, not from tb.h
    const float* schedule;         // [rows][row_floats]
    const int32_t* counter;
    int32_t* status;
    int32_t rows, row_floats, group_floats;        // group_floats: where this launch group's MAXH slots begin in a row
};
// the arguments of a plan prepared with STEP, without a schedule
StepArgs step_args(const gmpe_optim_plan* pl, const Layout& y);

// SCHED false: gmpe_optim_step's and gmpe_optim_step_shard's kernel (instantiated in gmpe_optim.hip), the Hyper sets in the kernel-argument table.
// SCHED true: gmpe_optim_step_scheduled's (gmpe_optim_sched.hip), the same lines on the sets of schedule row *counter; a counter outside 0 .. rows - 1
// touches no tensor, sets *status and still reports the norm.
template <bool SCHED>
__global__ __launch_bounds__(BLOCK) void k_opt_step(const Table tb, const StepArgs a) {
    __shared__ double red[BLOCK];
    double s = 0.0;
    for (int j = threadIdx.x; j < a.n_parts; j += BLOCK) s += a.part[j];
    const double norm = sqrt(block_sum(s, red));
    float coef = 1.0f;
    if (a.clip) {
        const double c = a.max_norm / (norm + 1e-6);
        coef = (float)(c > 1.0 ? 1.0 : c);                           // NaN stays NaN, as torch.clamp keeps it
    }
    const Hyper* hs = tb.h;
    bool spent = false;
    if (SCHED) {
        const int32_t row = *a.counter;                              // k_opt_advance, which writes it, is the call's last launch on this stream
        spent = row < 0 || row >= a.rows;
        hs = reinterpret_cast<const Hyper*>(a.schedule + (size_t)(spent ? 0 : row) * (size_t)a.row_floats + a.group_floats);
    }
    if (a.first && blockIdx.x == 0 && threadIdx.x == 0) {
        a.out[0] = norm; a.out[1] = (double)coef;
        if (a.norm_f32) a.norm_f32[0] = (float)norm;
        if (spent) *a.status = 1;
    }
    if (spent) return;
    const uint32_t e0 = blockIdx.x * (uint32_t)CHUNK + threadIdx.x;
    for (int k = 0; k < PER_THREAD; ++k) {
        const uint32_t e = e0 + (uint32_t)k * BLOCK;
        if (e >= tb.total) break;
        const Desc& d = tb.d[find_tensor(tb, e)];
        const uint32_t o = e - d.start;
        const bool scale = a.clip && (d.flags & GMPE_OPT_T_IN_NORM), step = a.step && (d.flags & GMPE_OPT_T_STEP);
        if (!scale && !step) continue;
        float g = d.g[o];
        if (scale) { g = g * coef; d.g[o] = g; }
        if (step) {
            const Hyper& h = hs[d.hyper];
            float p = d.p[o], m = d.m[o], v = d.v[o];
            if (h.wd != 0.0f) g = g + h.wd * p;
            m = m + (g - m) * h.w1;
            v = h.b2 * v + (h.w2 * g) * g;
            const float denom = sqrtf(v) / h.s2 + h.eps;
            p = p - h.a * (m / denom);
            d.m[o] = m; d.v[o] = v; d.p[o] = p;
        }
    }
}

// k_opt_step<SCHED> over every group (a table without elements: one launch that writes `out`)
template <bool SCHED>
int launch_step_groups(const Layout& y, StepArgs a, hipStream_t st) {
    for (size_t g = 0; g < y.groups.size(); ++g) {
        a.first = g == 0;
        a.group_floats = (int32_t)(g * MAXH * GMPE_OPT_HYPER_FLOATS);
        const int64_t grid = y.chunks[g] > 0 ? y.chunks[g] : (g == 0 ? 1 : 0);
        if (grid > 0) GMPE_LAUNCH(k_opt_step<SCHED>, dim3((unsigned)grid), dim3(BLOCK), 0, st, y.groups[g], a);
    }
    return GMPE_OK;
}

}  // namespace gmpe_opt
