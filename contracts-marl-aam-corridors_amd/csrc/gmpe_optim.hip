// gmpe_optim.hip — the gradient clip and the Adam step of GR_MAPPO.ppo_update over a table of tensors (include/gmpe.h gmpe_optim_step): the numeric
// contract, the geometry and the launch order are stated there, line by line. Two kernels per launch group of at most 64 tensors:
//   k_opt_norm  a chunk's double sum of exact squares -> part[chunk];
//   k_opt_step  every workgroup adds part[] itself in one fixed order (no finish kernel, no atomics: the list is a few hundred doubles at most for the
//               shipped networks and the sum costs less than a launch), then clips and steps its own chunk.
// The table is a kernel argument (64 descriptors of 40 bytes + 8 hyper-parameter sets of 28 bytes: under the 4 KB of a kernel's arguments), so a call
// uploads nothing, allocates nothing and waits for nothing. Sizes are tiny (about 41 000 elements for the shipped actor): the job is few launches, not
// bandwidth, which is why a lane finds its tensor by a binary search over the prefix sums rather than through a precomputed map in device memory.
// The table, the search, the workgroup sum and k_opt_step itself (a template, instantiated here with the sets in the kernel arguments) are
// gmpe_optim_table.h's, shared with gmpe_optim_shard.hip (gmpe_optim_step_shard), which launches this file's k_opt_step through launch_steps() behind its
// own sum kernel, and with gmpe_optim_sched.hip (gmpe_optim_step_scheduled), which instantiates it over a schedule in device memory.
#include <math.h>

#include "gmpe_optim_table.h"

using namespace gmpe_opt;

namespace {

__global__ __launch_bounds__(BLOCK) void k_opt_norm(const Table tb, double* __restrict__ part) {
    __shared__ double red[BLOCK];
    const uint32_t e0 = blockIdx.x * (uint32_t)CHUNK + threadIdx.x;
    double s = 0.0;
    for (int k = 0; k < PER_THREAD; ++k) {
        const uint32_t e = e0 + (uint32_t)k * BLOCK;
        if (e >= tb.total) break;
        const Desc& d = tb.d[find_tensor(tb, e)];
        if (d.flags & GMPE_OPT_T_IN_NORM) {
            const double g = (double)d.g[e - d.start];
            s += g * g;
        }
    }
    const double tot = block_sum(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

using gmpe::fail;

// what every entry point checks of the geometry: counts, numel, flags, hyper indices
int check_geometry(const char* fn, const gmpe_optim_plan* pl) {
    if (!pl) return fail(fn, "null plan");
    if (pl->n_tensors < 1 || pl->n_tensors > GMPE_OPT_MAX_PLAN_TENSORS) return fail(fn, "n_tensors must be in 1 .. " + std::to_string(GMPE_OPT_MAX_PLAN_TENSORS));
    if (pl->n_hypers < 0 || pl->n_hypers > GMPE_OPT_MAX_PLAN_TENSORS) return fail(fn, "n_hypers must be in 0 .. " + std::to_string(GMPE_OPT_MAX_PLAN_TENSORS));
    if (!pl->tensors) return fail(fn, "tensors is null");
    if (pl->n_hypers > 0 && !pl->hypers) return fail(fn, "hypers is null");
    for (int i = 0; i < pl->n_tensors; ++i) {
        const gmpe_optim_tensor& t = pl->tensors[i];
        const std::string at = "tensors[" + std::to_string(i) + "].";
        if (t.numel < 0 || t.numel > GMPE_OPT_MAX_NUMEL) return fail(fn, at + "numel must be in 0 .. 2^30");
        if (!(t.flags & (GMPE_OPT_T_IN_NORM | GMPE_OPT_T_STEP)) || (t.flags & ~(GMPE_OPT_T_IN_NORM | GMPE_OPT_T_STEP)))
            return fail(fn, at + "flags must be GMPE_OPT_T_IN_NORM, GMPE_OPT_T_STEP or both");
        if ((t.flags & GMPE_OPT_T_STEP) ? (t.hyper < 0 || t.hyper >= pl->n_hypers) : t.hyper != 0)
            return fail(fn, at + "hyper must index hypers with GMPE_OPT_T_STEP and be 0 without");
    }
    return GMPE_OK;
}

// The launch groups of a checked plan, filled as far as `depth` says: the geometry alone, with the pointers (GRADS), or with the pointers and the float32
// hyper-parameters (STEP).
void layout(const gmpe_optim_plan* pl, Depth depth, Layout& y) {
    int n_slots = 0;
    y.groups.emplace_back();
    y.slot_hyper.assign(MAXH, -1);
    int* slot_of = &y.slot_hyper[0];                                 // the plan's hyper index in each of the current group's slots
    Table* tb = &y.groups.back();
    tb->total = 0; tb->n = 0;
    for (int i = 0; i < pl->n_tensors; ++i) {
        const gmpe_optim_tensor& t = pl->tensors[i];
        if (t.numel == 0) continue;
        const bool steps = t.flags & GMPE_OPT_T_STEP;
        int slot = 0;
        if (steps) for (slot = 0; slot < n_slots && slot_of[slot] != t.hyper; ++slot) {}
        if (tb->n == MAXT || (steps && slot == MAXH) || (uint64_t)tb->total + (uint64_t)t.numel > GROUP_LIMIT) {
            y.groups.emplace_back();
            y.slot_hyper.resize(y.groups.size() * MAXH, -1);
            slot_of = &y.slot_hyper[(y.groups.size() - 1) * MAXH];
            tb = &y.groups.back();
            tb->total = 0; tb->n = 0; n_slots = 0; slot = 0;
        }
        if (steps && slot == n_slots) {
            slot_of[n_slots++] = t.hyper;
            if (depth == STEP) tb->h[slot] = make_hyper(pl->hypers[t.hyper], pl->hypers[t.hyper].t);
        }
        Desc& d = tb->d[tb->n++];
        d.start = tb->total; d.flags = (uint16_t)t.flags; d.hyper = (uint16_t)slot;
        if (depth != GEOMETRY) { d.p = t.param; d.g = t.grad; d.m = t.exp_avg; d.v = t.exp_avg_sq; }
        tb->total += (uint32_t)t.numel;
    }
    for (const Table& g : y.groups) {
        y.chunks.push_back(((int64_t)g.total + CHUNK - 1) / CHUNK);
        y.n_chunks += y.chunks.back();
        y.elems += (int64_t)g.total;
    }
    gmpe::Carver c;
    c.take((size_t)y.n_chunks * sizeof(double));
    y.total = c.total();
}

}  // namespace

int gmpe_opt::prepare(const char* fn, const gmpe_optim_plan* pl, Depth depth, Layout& y) {
    if (int rc = check_geometry(fn, pl)) return rc;
    if (depth == GRADS) {
        for (int i = 0; i < pl->n_tensors; ++i)
            if (int rc = gmpe::check_ptr(fn, pl->tensors[i].grad, "tensors[" + std::to_string(i) + "].grad", pl->tensors[i].numel > 0)) return rc;
    } else if (depth == STEP) {
        if (pl->flags & ~(GMPE_OPT_CLIP | GMPE_OPT_STEP)) return fail(fn, "flags must be GMPE_OPT_CLIP, GMPE_OPT_STEP, both or 0");
        if (pl->reserved != 0) return fail(fn, "reserved must be 0");
        const bool clip = pl->flags & GMPE_OPT_CLIP, step = pl->flags & GMPE_OPT_STEP;
        if (int rc = check_hypers(fn, pl)) return rc;
        if (clip && !(pl->max_norm > 0.0)) return fail(fn, "max_norm must be > 0 with GMPE_OPT_CLIP");
        for (int i = 0; i < pl->n_tensors; ++i) {
            const gmpe_optim_tensor& t = pl->tensors[i];
            const bool steps = step && (t.flags & GMPE_OPT_T_STEP) && t.numel > 0;          // an empty tensor has no address
            const gmpe::PtrField ps[] = {{t.param, "param", steps}, {t.grad, "grad", t.numel > 0}, {t.exp_avg, "exp_avg", steps}, {t.exp_avg_sq, "exp_avg_sq", steps}};
            if (int rc = gmpe::check_ptrs(fn, ps, "tensors[" + std::to_string(i) + "].")) return rc;
        }
        if (!pl->out) return fail(fn, "out is required");
        if ((uintptr_t)pl->out & 7) return fail(fn, "out must be 8-byte aligned");
        if (int rc = gmpe::check_ptr(fn, pl->grad_norm_f32, "grad_norm_f32", false)) return rc;
    }
    layout(pl, depth, y);
    if (y.n_chunks > 0x7fffffffLL) return fail(fn, "tensors: too many elements for one call");
    if (depth == STEP)
        return gmpe::check_workspace(fn, pl->workspace, pl->workspace_bytes, y.total, y.total > 0, "workspace is required", "gmpe_optim_workspace_bytes(plan)");
    return GMPE_OK;
}

int gmpe_opt::check_hypers(const char* fn, const gmpe_optim_plan* pl) {
    for (int i = 0; i < pl->n_hypers; ++i) {
        const gmpe_optim_hyper& h = pl->hypers[i];
        const std::string at = "hypers[" + std::to_string(i) + "].";
        if (!(h.lr >= 0.0)) return fail(fn, at + "lr must be >= 0");
        if (!(h.beta1 >= 0.0 && h.beta1 < 1.0)) return fail(fn, at + "beta1 must be in [0, 1)");
        if (!(h.beta2 >= 0.0 && h.beta2 < 1.0)) return fail(fn, at + "beta2 must be in [0, 1)");
        if (!(h.eps >= 0.0)) return fail(fn, at + "eps must be >= 0");
        if (!(h.weight_decay >= 0.0)) return fail(fn, at + "weight_decay must be >= 0");
        if (h.t < 1) return fail(fn, at + "t must be >= 1");
    }
    return GMPE_OK;
}

int gmpe_opt::launch_norms(const gmpe_optim_plan* pl, const Layout& y, hipStream_t st) {
    double* part = static_cast<double*>(pl->workspace);
    int64_t base = 0;
    for (size_t g = 0; g < y.groups.size(); ++g) {
        if (y.chunks[g] > 0) GMPE_LAUNCH(k_opt_norm, dim3((unsigned)y.chunks[g]), dim3(BLOCK), 0, st, y.groups[g], part + base);
        base += y.chunks[g];
    }
    return GMPE_OK;
}

gmpe_opt::StepArgs gmpe_opt::step_args(const gmpe_optim_plan* pl, const Layout& y) {
    return StepArgs{static_cast<const double*>(pl->workspace), (int32_t)y.n_chunks, (pl->flags & GMPE_OPT_CLIP) != 0, (pl->flags & GMPE_OPT_STEP) != 0, 0,
                    pl->max_norm, pl->out, pl->grad_norm_f32, nullptr, nullptr, nullptr, 0, 0, 0};
}

int gmpe_opt::launch_steps(const gmpe_optim_plan* pl, const Layout& y, hipStream_t st) { return launch_step_groups<false>(y, step_args(pl, y), st); }

gmpe_opt::Hyper gmpe_opt::make_hyper(const gmpe_optim_hyper& h, int64_t t) {
    const double bc1 = 1.0 - pow(h.beta1, (double)t), bc2 = 1.0 - pow(h.beta2, (double)t);
    return Hyper{(float)h.weight_decay, (float)(1.0 - h.beta1), (float)h.beta2, (float)(1.0 - h.beta2), (float)(h.lr / bc1), (float)sqrt(bc2), (float)h.eps};
}

extern "C" {

int gmpe_optim_workspace_bytes(const gmpe_optim_plan* pl, size_t* bytes_out) {
    const char* fn = "gmpe_optim_workspace_bytes";
    if (!bytes_out) return fail(fn, "bytes_out is null");
    Layout y;
    if (int rc = prepare(fn, pl, GEOMETRY, y)) return rc;
    *bytes_out = y.total;
    return GMPE_OK;
}

int gmpe_optim_step(int device, const gmpe_optim_plan* pl, void* stream) {
    Layout y;
    if (int rc = prepare("gmpe_optim_step", pl, STEP, y)) return rc;
    GMPE_HIP_CHECK(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = launch_norms(pl, y, st)) return rc;
    return launch_steps(pl, y, st);
}

}  // extern "C"
