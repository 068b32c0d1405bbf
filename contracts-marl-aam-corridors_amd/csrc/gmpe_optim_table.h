// gmpe_optim_table.h — what gmpe_optim.hip (gmpe_optim_step) and gmpe_optim_shard.hip (gmpe_optim_step_shard) share (internal: not installed): the table
// of tensors that travels as a kernel argument, the search of an element's tensor, the workgroup sum, and the host half that checks a plan, cuts it into
// launch groups and launches k_opt_step. The host functions are defined once, in gmpe_optim.hip.
#pragma once
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

}  // namespace gmpe_opt
