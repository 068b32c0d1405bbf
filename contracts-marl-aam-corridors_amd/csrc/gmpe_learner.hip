// gmpe_learner.hip — the learner's fields of one rollout step (include/gmpe.h gmpe_insert_learner): what GMPERunner.insert hands
// GraphReplayBuffer.insert from the policy (onpolicy/runner/shared/graph_mpe_runner.py:384-392, onpolicy/utils/graph_buffer.py:229-234), written
// into the device buffer's slots in one launch. Handle-less: the buffer's slots and the policy's outputs are all it needs.
//
// k_insert_learner: one workgroup per LI_LANES consecutive lanes. The workgroup reads its lanes' dones once into LDS, copies the per-lane
// values / actions / log-probs, then the [lanes, R, H] rows of both RNN states, a done lane's row stored as zeros (the runner's
// `rnn_states[dones] = 0`; a done lane's input row is not read). The rows of a workgroup's lanes are one contiguous range of the input and of
// the destination slot, so the copy is a flat loop over it: 16-byte units when the row length is a multiple of 4 floats and both ends are 16-byte
// aligned, 4-byte units otherwise. Each thread loads LI_UNROLL units before it stores them. Plain stores: the next policy call reads slot t + 1.
//
// k_step_tail (gmpe_step_tail): the same workgroups and the same learner rows (learner_rows, shared by both kernels), and with them everything else that
// follows an env step and is a function of dones[t - 1], dones[t] alone: masks[t + 1] / active_masks[t + 1] (k_masks' rule, gmpe_step.hip), the stop rows
// of position t of available_actions (k_stop_actions' rule, gmpe_returns.hip) and the action draw counter's advance (one thread of workgroup 0).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "gmpe_host.h"          // include/gmpe.h, the error text, GMPE_HIP_CHECK

namespace {

constexpr int LI_BLOCK = 256;
constexpr int LI_LANES = 32;      // lanes per workgroup: at c2 (R*H = 64) 2 x 512 16-byte units per workgroup, 1280 workgroups
constexpr int LI_UNROLL = 4;      // units each thread has in flight

struct RnnRows {
    const float* src;    // [lanes, row] input, or null (field skipped)
    float* dst;          // slot t + 1
    uint32_t row;        // R * H floats
    int32_t vec;         // 1: 16-byte units
};

struct LiArgs {
    int64_t lanes;
    int32_t k, a64;
    const uint8_t* done;              // dones[t], or null (no RNN field)
    const float* v_in;
    float* v_out;
    const void* a_in;
    float* a_out;
    const float* lp_in;
    float* lp_out;
    RnnRows rnn[2];
};

// n units of U (float4 or float) from s to d, unit i belonging to lane i / per_lane of the workgroup; done lanes get zeros, their input unread.
template <typename U>
__device__ __forceinline__ void copy_rows(const U* s, U* d, uint32_t n, uint32_t per_lane, const uint8_t* done_sh) {
    const U zero{};
    for (uint32_t base = threadIdx.x; base < n; base += LI_BLOCK * LI_UNROLL) {
        U v[LI_UNROLL];
#pragma unroll
        for (int u = 0; u < LI_UNROLL; ++u) {
            const uint32_t i = base + u * LI_BLOCK;
            v[u] = zero;
            if (i < n && !done_sh[i / per_lane]) v[u] = s[i];
        }
#pragma unroll
        for (int u = 0; u < LI_UNROLL; ++u) {
            const uint32_t i = base + u * LI_BLOCK;
            if (i < n) d[i] = v[u];
        }
    }
}

__device__ __forceinline__ void rnn_rows(const RnnRows& r, int64_t lane0, int nl, const uint8_t* done_sh) {
    if (!r.src) return;
    const int64_t off = lane0 * r.row;
    if (r.vec) {
        const uint32_t per = r.row >> 2;
        copy_rows(reinterpret_cast<const float4*>(r.src + off), reinterpret_cast<float4*>(r.dst + off), (uint32_t)nl * per, per, done_sh);
    } else {
        copy_rows(r.src + off, r.dst + off, (uint32_t)nl * r.row, r.row, done_sh);
    }
}

// The per-lane fields of the workgroup's nl lanes from lane0 on: values, actions, log-probs
__device__ __forceinline__ void learner_lanes(const LiArgs& p, int64_t lane0, int nl) {
    const int tid = threadIdx.x;
    if (p.v_in && tid < nl) p.v_out[lane0 + tid] = p.v_in[lane0 + tid];
    const int nk = nl * p.k;
    for (int i = tid; i < nk; i += LI_BLOCK) {
        const int64_t o = lane0 * p.k + i;
        // GraphReplayBuffer stores the policy's int64 actions in a float32 array: NumPy's int64 -> float32 cast, round to nearest
        if (p.a_in) p.a_out[o] = p.a64 ? (float)static_cast<const int64_t*>(p.a_in)[o] : static_cast<const float*>(p.a_in)[o];
        if (p.lp_in) p.lp_out[o] = p.lp_in[o];
    }
}

__global__ __launch_bounds__(LI_BLOCK) void k_insert_learner(LiArgs p) {
    __shared__ uint8_t done_sh[LI_LANES];
    const int64_t lane0 = (int64_t)blockIdx.x * LI_LANES;
    const int64_t left = p.lanes - lane0;
    const int nl = left < LI_LANES ? (int)left : LI_LANES;
    const int tid = threadIdx.x;
    if (p.done && tid < nl) done_sh[tid] = p.done[lane0 + tid];
    learner_lanes(p, lane0, nl);
    if (!p.done) return;                                    // uniform: no RNN field
    __syncthreads();
    rnn_rows(p.rnn[0], lane0, nl, done_sh);
    rnn_rows(p.rnn[1], lane0, nl, done_sh);
}

struct TailArgs {
    LiArgs li;                        // li.done: dones[t], always set
    const uint8_t* done_prev;         // dones[t - 1], or null at t = 0 (stop rows all ones)
    float* masks;                     // slot t + 1, or null
    float* active;                    // slot t + 1, or null
    float* avail;                     // position t: [lanes, n] rows, or null
    int32_t A, n;
    uint64_t* draw_dev;
    uint64_t draw_inc;
};

__global__ __launch_bounds__(LI_BLOCK) void k_step_tail(TailArgs p) {
    __shared__ uint8_t done_sh[LI_LANES];
    const int64_t lane0 = (int64_t)blockIdx.x * LI_LANES;
    const int64_t left = p.li.lanes - lane0;
    const int nl = left < LI_LANES ? (int)left : LI_LANES;
    const int tid = threadIdx.x;
    if (tid < nl) {
        const int64_t q = lane0 + tid;
        const bool d = p.li.done[q] != 0;
        done_sh[tid] = d;
        if (p.masks) p.masks[q] = d ? 0.0f : 1.0f;
        if (p.active) {
            // an env's A lanes may lie in two workgroups: the all-done test reads the env's bytes from memory, not from done_sh
            const int64_t q0 = q / p.A * p.A;
            bool all = true;
            for (int a = 0; a < p.A; ++a) all = all && p.li.done[q0 + a] != 0;
            p.active[q] = (d && !all) ? 0.0f : 1.0f;
        }
    }
    if (blockIdx.x == 0 && tid == LI_BLOCK - 1 && p.draw_dev) *p.draw_dev += p.draw_inc;     // the step's sampling launch has read it
    if (p.avail) {
        const int n = p.n, nn = nl * n;
        for (int i = tid; i < nn; i += LI_BLOCK) {
            const int lane = i / n, j = i - lane * n;
            float v = 1.0f;
            if (p.done_prev && p.done_prev[lane0 + lane]) v = j == n / 2 ? 1.0f : 0.0f;          // available_actions[int(n / 2)] = 1
            p.avail[lane0 * n + i] = v;
        }
    }
    learner_lanes(p.li, lane0, nl);
    __syncthreads();
    rnn_rows(p.li.rnn[0], lane0, nl, done_sh);
    rnn_rows(p.li.rnn[1], lane0, nl, done_sh);
}

int fail(const char* fn, const std::string& m) { return gmpe::report_error(GMPE_ERR_INVALID_ARG, std::string(fn) + ": " + m); }

bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// The checks of gmpe_insert_learner, shared with gmpe_step_tail (`fn`: the entry's name)
int check_learner_plan(const char* fn, const gmpe_learner_plan* pl) {
    if (pl->lanes < 1) return fail(fn, "need lanes >= 1");
    if (pl->num_steps < 1 || pl->t < 0 || pl->t >= pl->num_steps) return fail(fn, "need num_steps >= 1 and 0 <= t < num_steps");
    if (pl->reserved != 0 || (pl->actions_int64 != 0 && pl->actions_int64 != 1)) return fail(fn, "actions_int64 must be 0 or 1 and reserved 0");
    const bool rnn = pl->rnn_in, rnnc = pl->rnn_critic_in, ak = pl->actions_in || pl->log_probs_in;
    if ((rnn || rnnc) && (pl->recurrent_n < 1 || pl->recurrent_n > 64)) return fail(fn, "recurrent_n must be in 1 .. 64");
    if ((rnn && (pl->hidden < 1 || pl->hidden > 65536)) || (rnnc && (pl->hidden_critic < 1 || pl->hidden_critic > 65536)))
        return fail(fn, "hidden / hidden_critic must be in 1 .. 65536");
    if (ak && (pl->act_dim < 1 || pl->act_dim > 64)) return fail(fn, "act_dim must be in 1 .. 64");
    if ((pl->values && !pl->value_preds) || (pl->actions_in && !pl->actions) || (pl->log_probs_in && !pl->action_log_probs) ||
        (rnn && !pl->rnn_states) || (rnnc && !pl->rnn_states_critic))
        return fail(fn, "an input is given without its output array");
    if ((rnn || rnnc) && !pl->dones) return fail(fn, "the RNN states need dones");
    const int64_t L = pl->lanes, k = pl->act_dim, R = pl->recurrent_n;
    const int64_t row = R * pl->hidden, rowc = R * pl->hidden_critic;
    const void* f32s[] = {pl->values, pl->log_probs_in, pl->rnn_in, pl->rnn_critic_in, pl->value_preds, pl->actions, pl->action_log_probs,
                          pl->rnn_states, pl->rnn_states_critic};
    for (const void* q : f32s)
        if (!aligned(q, 4)) return fail(fn, "misaligned pointer: float32 arrays need 4-byte alignment");
    if (!aligned(pl->actions_in, pl->actions_int64 ? 8 : 4)) return fail(fn, "misaligned pointer: actions_in needs the alignment of its type");
    // every used array: a slot is at least as long as the rows it receives, so slots t and t + 1 do not overlap
    if (((rnn || rnnc) && pl->stride_dones < L) || (pl->values && pl->stride_value_preds < L) || (pl->actions_in && pl->stride_actions < L * k) ||
        (pl->log_probs_in && pl->stride_action_log_probs < L * k) || (rnn && pl->stride_rnn_states < L * row) ||
        (rnnc && pl->stride_rnn_states_critic < L * rowc))
        return fail(fn, "misaligned or overlapping strides: every stride must be at least one slot (lanes x row elements)");
    if ((L + LI_LANES - 1) / LI_LANES > 0x7fffffffLL) return fail(fn, "too many lanes for one launch");
    return GMPE_OK;
}

// The kernel's view of a checked plan; dones[t] only where the plan has dones
LiArgs learner_args(const gmpe_learner_plan* pl) {
    LiArgs a{};
    const bool rnn = pl->rnn_in, rnnc = pl->rnn_critic_in;
    const int64_t t = pl->t, row = (int64_t)pl->recurrent_n * pl->hidden, rowc = (int64_t)pl->recurrent_n * pl->hidden_critic;
    a.lanes = pl->lanes; a.k = pl->act_dim; a.a64 = pl->actions_int64;
    a.done = pl->dones ? pl->dones + t * pl->stride_dones : nullptr;
    if (pl->values) { a.v_in = pl->values; a.v_out = pl->value_preds + t * pl->stride_value_preds; }
    if (pl->actions_in) { a.a_in = pl->actions_in; a.a_out = pl->actions + t * pl->stride_actions; }
    if (pl->log_probs_in) { a.lp_in = pl->log_probs_in; a.lp_out = pl->action_log_probs + t * pl->stride_action_log_probs; }
    const float* srcs[2] = {pl->rnn_in, pl->rnn_critic_in};
    float* dsts[2] = {rnn ? pl->rnn_states + (t + 1) * pl->stride_rnn_states : nullptr,
                      rnnc ? pl->rnn_states_critic + (t + 1) * pl->stride_rnn_states_critic : nullptr};
    const int64_t rows[2] = {row, rowc};
    for (int f = 0; f < 2; ++f) {
        if (!srcs[f]) continue;
        a.rnn[f].src = srcs[f];
        a.rnn[f].dst = dsts[f];
        a.rnn[f].row = (uint32_t)rows[f];
        a.rnn[f].vec = rows[f] % 4 == 0 && aligned(srcs[f], 16) && aligned(dsts[f], 16);
    }
    return a;
}

unsigned num_blocks(int64_t lanes) { return (unsigned)((lanes + LI_LANES - 1) / LI_LANES); }

}  // namespace

extern "C" int gmpe_insert_learner(int device, const gmpe_learner_plan* pl, void* stream) {
    const char* fn = "gmpe_insert_learner";
    if (!pl) return fail(fn, "null plan");
    if (int rc = check_learner_plan(fn, pl)) return rc;
    const bool rnn = pl->rnn_in || pl->rnn_critic_in;
    if (!pl->values && !pl->actions_in && !pl->log_probs_in && !rnn) return GMPE_OK;
    LiArgs a = learner_args(pl);
    if (!rnn) a.done = nullptr;                             // read only for the RNN rows
    GMPE_HIP_CHECK(hipSetDevice(device));
    hipLaunchKernelGGL(k_insert_learner, dim3(num_blocks(pl->lanes)), dim3(LI_BLOCK), 0, static_cast<hipStream_t>(stream), a);
    GMPE_HIP_CHECK(hipGetLastError());
    return GMPE_OK;
}

extern "C" int gmpe_step_tail(int device, const gmpe_step_tail_plan* tp, void* stream) {
    const char* fn = "gmpe_step_tail";
    if (!tp) return fail(fn, "null plan");
    const gmpe_learner_plan* pl = &tp->learner;
    if (int rc = check_learner_plan(fn, pl)) return rc;
    const int64_t L = pl->lanes;
    if (!pl->dones) return fail(fn, "dones is required: the masks read it");
    if (tp->num_agents < 1 || L % tp->num_agents != 0) return fail(fn, "need num_agents >= 1 and lanes % num_agents == 0");
    if (tp->available_actions && (tp->n_actions < 1 || tp->n_actions > 64)) return fail(fn, "n_actions must be in 1 .. 64");
    if (!aligned(tp->masks, 4) || !aligned(tp->active_masks, 4) || !aligned(tp->available_actions, 4))
        return fail(fn, "misaligned pointer: float32 arrays need 4-byte alignment");
    if (!aligned(tp->draw_dev, 8)) return fail(fn, "misaligned pointer: draw_dev needs 8-byte alignment");
    if (pl->stride_dones < L || (tp->masks && tp->stride_masks < L) || (tp->active_masks && tp->stride_active_masks < L) ||
        (tp->available_actions && tp->stride_available_actions < L * tp->n_actions))
        return fail(fn, "misaligned or overlapping strides: every stride must be at least one slot (lanes x row elements)");
    TailArgs a{};
    const int64_t t = pl->t;
    a.li = learner_args(pl);
    a.done_prev = t > 0 ? pl->dones + (t - 1) * pl->stride_dones : nullptr;
    a.masks = tp->masks ? tp->masks + (t + 1) * tp->stride_masks : nullptr;
    a.active = tp->active_masks ? tp->active_masks + (t + 1) * tp->stride_active_masks : nullptr;
    a.avail = tp->available_actions ? tp->available_actions + t * tp->stride_available_actions : nullptr;
    a.A = tp->num_agents; a.n = tp->n_actions;
    a.draw_dev = tp->draw_dev; a.draw_inc = tp->draw_inc;
    GMPE_HIP_CHECK(hipSetDevice(device));
    hipLaunchKernelGGL(k_step_tail, dim3(num_blocks(L)), dim3(LI_BLOCK), 0, static_cast<hipStream_t>(stream), a);
    GMPE_HIP_CHECK(hipGetLastError());
    return GMPE_OK;
}
