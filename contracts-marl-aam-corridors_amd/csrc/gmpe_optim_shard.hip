// gmpe_optim_shard.hip — gmpe_optim_step for a learner whose minibatch lies in `world` shards (include/gmpe.h gmpe_optim_step_shard): the clip and the
// step work on the sum over the shards of their gradients, taken in shard order in double and rounded once. Two phases around one all-gather:
//   GMPE_SHARD_LOCAL   k_opt_pack    every gradient of the table copied back to back into `local`; nothing else is touched;
//   GMPE_SHARD_APPLY   k_opt_reduce  in place of k_opt_norm: an element's `world` values of `all` added, the sum written to the tensor's own grad, the
//                                    chunk's double sum of exact squares -> part[chunk] in k_opt_norm's layout and order;
//                      k_opt_step    gmpe_optim.hip's, unchanged.
// The table, the search and the host half are gmpe_optim_table.h's: nothing is uploaded, allocated or waited for, and there are no atomics.
#include "gmpe_optim_table.h"

using namespace gmpe_opt;

namespace {

constexpr int ROWS = 8;            // the shards whose values of a thread's four elements are in flight together: 32 loads before the first add

// local: the group's first element in the packed array
__global__ __launch_bounds__(BLOCK) void k_opt_pack(const Table tb, float* __restrict__ local) {
    const uint32_t e0 = blockIdx.x * (uint32_t)CHUNK + threadIdx.x;
    for (int k = 0; k < PER_THREAD; ++k) {
        const uint32_t e = e0 + (uint32_t)k * BLOCK;
        if (e >= tb.total) break;
        const Desc& d = tb.d[find_tensor(tb, e)];
        local[e] = d.g[e - d.start];
    }
}

// all: the group's first element in shard 0's row; n: the elements of a row
__global__ __launch_bounds__(BLOCK) void k_opt_reduce(const Table tb, const float* __restrict__ all, const int world, const size_t n, double* __restrict__ part) {
    __shared__ double red[BLOCK];
    const uint32_t e0 = blockIdx.x * (uint32_t)CHUNK + threadIdx.x;
    double acc[PER_THREAD];
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) acc[k] = 0.0;
    for (int r0 = 0; r0 < world; r0 += ROWS) {
        float x[PER_THREAD][ROWS];
#pragma unroll
        for (int k = 0; k < PER_THREAD; ++k) {
            const uint32_t e = e0 + (uint32_t)k * BLOCK;
#pragma unroll
            for (int j = 0; j < ROWS; ++j) x[k][j] = (e < tb.total && r0 + j < world) ? all[(size_t)(r0 + j) * n + e] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < PER_THREAD; ++k) {
#pragma unroll
            for (int j = 0; j < ROWS; ++j)
                if (r0 + j < world) acc[k] = (r0 + j == 0) ? (double)x[k][j] : acc[k] + (double)x[k][j];      // the fold starts AT shard 0: -0 stays -0
        }
    }
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const uint32_t e = e0 + (uint32_t)k * BLOCK;
        if (e < tb.total) {
            const Desc& d = tb.d[find_tensor(tb, e)];
            const float g = (float)acc[k];
            d.g[e - d.start] = g;
            if (d.flags & GMPE_OPT_T_IN_NORM) s += (double)g * (double)g;
        }
    }
    const double tot = block_sum(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

using gmpe::fail;

}  // namespace

extern "C" {

int gmpe_optim_shard_elems(const gmpe_optim_plan* pl, int64_t* elems_out) {
    const char* fn = "gmpe_optim_shard_elems";
    if (!elems_out) return fail(fn, "elems_out is null");
    Layout y;
    if (int rc = prepare(fn, pl, GEOMETRY, y)) return rc;
    *elems_out = y.elems;
    return GMPE_OK;
}

int gmpe_optim_step_shard(int device, const gmpe_optim_shard_plan* sp, void* stream) {
    const char* fn = "gmpe_optim_step_shard";
    if (!sp) return fail(fn, "null plan");
    if (sp->phase != GMPE_SHARD_LOCAL && sp->phase != GMPE_SHARD_APPLY) return fail(fn, "phase must be GMPE_SHARD_LOCAL or GMPE_SHARD_APPLY");
    if (sp->world < 1 || sp->world > GMPE_SHARD_MAX_WORLD) return fail(fn, "world must be in 1 .. " + std::to_string(GMPE_SHARD_MAX_WORLD));
    const bool apply = sp->phase == GMPE_SHARD_APPLY;
    if (apply ? (!sp->all || ((uintptr_t)sp->all & 3)) : (!sp->local || ((uintptr_t)sp->local & 3)))
        return fail(fn, apply ? "all is required with GMPE_SHARD_APPLY: f32 device memory, 4-byte aligned" : "local is required with GMPE_SHARD_LOCAL: f32 device memory, 4-byte aligned");
    Layout y;
    if (int rc = prepare(fn, &sp->base, apply ? STEP : GRADS, y)) return rc;
    if (sp->local_elems != y.elems) return fail(fn, "local_elems must be gmpe_optim_shard_elems(&base) = " + std::to_string(y.elems));
    if ((int64_t)sp->world * sp->local_elems > 0x7fffffffLL) return fail(fn, "world * local_elems must not exceed 2^31 - 1");
    GMPE_HIP_CHECK(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* part = static_cast<double*>(sp->base.workspace);
    int64_t first = 0, chunk = 0;          // the group's first element in a row, its first chunk
    for (size_t g = 0; g < y.groups.size(); ++g) {
        if (y.chunks[g] > 0) {
            if (apply)
                GMPE_LAUNCH(k_opt_reduce, dim3((unsigned)y.chunks[g]), dim3(BLOCK), 0, st, y.groups[g], sp->all + first, (int)sp->world, (size_t)sp->local_elems,
                            part + chunk);
            else
                GMPE_LAUNCH(k_opt_pack, dim3((unsigned)y.chunks[g]), dim3(BLOCK), 0, st, y.groups[g], sp->local + first);
        }
        first += (int64_t)y.groups[g].total;
        chunk += y.chunks[g];
    }
    return apply ? launch_steps(&sp->base, y, st) : GMPE_OK;
}

}  // extern "C"
