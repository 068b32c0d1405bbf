// gmpe_optim_sched.hip — gmpe_optim_step with Adam's step count in device memory (include/gmpe.h gmpe_optim_schedule_bytes / _fill,
// gmpe_optim_step_scheduled), so that a captured graph of the step can be replayed: the float32 hyper-parameter sets of `rows` consecutive step counts
// lie in a schedule on the device, a device counter picks the row, and the call's last launch advances it. The checks, the launch groups, k_opt_norm and
// the rounding of a set (make_hyper) are gmpe_optim.hip's; the step kernel is gmpe_optim_table.h's k_opt_step, instantiated here to take its sets from
// schedule[*counter] — no second copy of the arithmetic. The kernel arguments do not depend on the step count.
#include "gmpe_optim_table.h"

using namespace gmpe_opt;
using gmpe::fail;

namespace {

// the last launch of gmpe_optim_step_scheduled: every k_opt_step of the call has read the counter before this writes it (same stream)
__global__ void k_opt_advance(int32_t* counter, int32_t rows) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int32_t row = *counter;
        if (row >= 0 && row < rows) *counter = row + 1;
    }
}

int check_rows(const char* fn, int32_t rows) {
    if (rows < 1 || rows > GMPE_OPT_MAX_SCHEDULE_ROWS) return fail(fn, "rows must be in 1 .. " + std::to_string(GMPE_OPT_MAX_SCHEDULE_ROWS));
    return GMPE_OK;
}

}  // namespace

extern "C" {

int gmpe_optim_schedule_bytes(const gmpe_optim_plan* pl, int32_t rows, size_t* bytes_out) {
    const char* fn = "gmpe_optim_schedule_bytes";
    if (!bytes_out) return fail(fn, "bytes_out is null");
    Layout y;
    if (int rc = prepare(fn, pl, GEOMETRY, y)) return rc;
    if (int rc = check_rows(fn, rows)) return rc;
    *bytes_out = (size_t)rows * y.groups.size() * MAXH * sizeof(Hyper);
    return GMPE_OK;
}

int gmpe_optim_schedule_fill(const gmpe_optim_plan* pl, int32_t rows, void* host_dst) {
    const char* fn = "gmpe_optim_schedule_fill";
    Layout y;
    if (int rc = prepare(fn, pl, GEOMETRY, y)) return rc;
    if (int rc = check_rows(fn, rows)) return rc;
    if (int rc = check_hypers(fn, pl)) return rc;
    if (int rc = gmpe::check_ptr(fn, host_dst, "host_dst", true)) return rc;
    Hyper* dst = static_cast<Hyper*>(host_dst);
    const size_t slots = y.slot_hyper.size();                        // groups * MAXH: one row
    for (int32_t k = 0; k < rows; ++k)
        for (size_t s = 0; s < slots; ++s) {
            const int i = y.slot_hyper[s];
            dst[(size_t)k * slots + s] = i < 0 ? Hyper{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f} : make_hyper(pl->hypers[i], pl->hypers[i].t + k);
        }
    return GMPE_OK;
}

int gmpe_optim_step_scheduled(int device, const gmpe_optim_sched_plan* sp, void* stream) {
    const char* fn = "gmpe_optim_step_scheduled";
    if (!sp) return fail(fn, "null plan");
    const gmpe_optim_plan* pl = &sp->base;
    Layout y;
    if (int rc = prepare(fn, pl, STEP, y)) return rc;
    if (int rc = check_rows(fn, sp->rows)) return rc;
    if (sp->reserved != 0) return fail(fn, "reserved must be 0");
    if ((pl->flags & GMPE_OPT_STEP) && !sp->schedule) return fail(fn, "schedule is required with GMPE_OPT_STEP");
    const gmpe::PtrField ps[] = {{sp->schedule, "schedule", false}, {sp->counter, "counter", true}, {sp->status, "status", true}};
    if (int rc = gmpe::check_ptrs(fn, ps)) return rc;
    GMPE_HIP_CHECK(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = launch_norms(pl, y, st)) return rc;
    StepArgs a = step_args(pl, y);
    a.schedule = sp->schedule; a.counter = sp->counter; a.status = sp->status; a.rows = sp->rows;
    a.row_floats = (int32_t)(y.groups.size() * MAXH * GMPE_OPT_HYPER_FLOATS);
    if (int rc = launch_step_groups<true>(y, a, st)) return rc;
    GMPE_LAUNCH(k_opt_advance, dim3(1), dim3(1), 0, st, sp->counter, sp->rows);
    return GMPE_OK;
}

}  // extern "C"
