// gmpe_learner.hip — the learner's fields of one rollout step (include/gmpe.h gmpe_insert_learner): what GMPERunner.insert hands
// GraphReplayBuffer.insert from the policy (onpolicy/runner/shared/graph_mpe_runner.py:384-392, onpolicy/utils/graph_buffer.py:229-234), written
// into the device buffer's slots in one launch. Handle-less: the buffer's slots and the policy's outputs are all it needs.
//
// k_insert_learner: one workgroup per LI_LANES consecutive lanes. The workgroup reads its lanes' dones once into LDS, copies the per-lane
// values / actions / log-probs, then the [lanes, R, H] rows of both RNN states, a done lane's row stored as zeros (the runner's
// `rnn_states[dones] = 0`; a done lane's input row is not read). The rows of a workgroup's lanes are one contiguous range of the input and of
// the destination slot, so the copy is a flat loop over it: 16-byte units when the row length is a multiple of 4 floats and both ends are 16-byte
// aligned, 4-byte units otherwise. Each thread loads LI_UNROLL units before it stores them. Plain stores: the next policy call reads slot t + 1.
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

__global__ __launch_bounds__(LI_BLOCK) void k_insert_learner(LiArgs p) {
    __shared__ uint8_t done_sh[LI_LANES];
    const int64_t lane0 = (int64_t)blockIdx.x * LI_LANES;
    const int64_t left = p.lanes - lane0;
    const int nl = left < LI_LANES ? (int)left : LI_LANES;
    const int tid = threadIdx.x;
    if (p.done && tid < nl) done_sh[tid] = p.done[lane0 + tid];
    if (p.v_in && tid < nl) p.v_out[lane0 + tid] = p.v_in[lane0 + tid];
    const int nk = nl * p.k;
    for (int i = tid; i < nk; i += LI_BLOCK) {
        const int64_t o = lane0 * p.k + i;
        // GraphReplayBuffer stores the policy's int64 actions in a float32 array: NumPy's int64 -> float32 cast, round to nearest
        if (p.a_in) p.a_out[o] = p.a64 ? (float)static_cast<const int64_t*>(p.a_in)[o] : static_cast<const float*>(p.a_in)[o];
        if (p.lp_in) p.lp_out[o] = p.lp_in[o];
    }
    if (!p.done) return;                                    // uniform: no RNN field
    __syncthreads();
    rnn_rows(p.rnn[0], lane0, nl, done_sh);
    rnn_rows(p.rnn[1], lane0, nl, done_sh);
}

int fail(const std::string& m) { return gmpe::report_error(GMPE_ERR_INVALID_ARG, "gmpe_insert_learner: " + m); }

bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" int gmpe_insert_learner(int device, const gmpe_learner_plan* pl, void* stream) {
    if (!pl) return fail("null plan");
    if (pl->lanes < 1) return fail("need lanes >= 1");
    if (pl->num_steps < 1 || pl->t < 0 || pl->t >= pl->num_steps) return fail("need num_steps >= 1 and 0 <= t < num_steps");
    if (pl->reserved != 0 || (pl->actions_int64 != 0 && pl->actions_int64 != 1)) return fail("actions_int64 must be 0 or 1 and reserved 0");
    const bool rnn = pl->rnn_in, rnnc = pl->rnn_critic_in, ak = pl->actions_in || pl->log_probs_in;
    if ((rnn || rnnc) && (pl->recurrent_n < 1 || pl->recurrent_n > 64)) return fail("recurrent_n must be in 1 .. 64");
    if ((rnn && (pl->hidden < 1 || pl->hidden > 65536)) || (rnnc && (pl->hidden_critic < 1 || pl->hidden_critic > 65536)))
        return fail("hidden / hidden_critic must be in 1 .. 65536");
    if (ak && (pl->act_dim < 1 || pl->act_dim > 64)) return fail("act_dim must be in 1 .. 64");
    if ((pl->values && !pl->value_preds) || (pl->actions_in && !pl->actions) || (pl->log_probs_in && !pl->action_log_probs) ||
        (rnn && !pl->rnn_states) || (rnnc && !pl->rnn_states_critic))
        return fail("an input is given without its output array");
    if ((rnn || rnnc) && !pl->dones) return fail("the RNN states need dones");
    const int64_t L = pl->lanes, k = pl->act_dim, R = pl->recurrent_n;
    const int64_t row = R * pl->hidden, rowc = R * pl->hidden_critic;
    const void* f32s[] = {pl->values, pl->log_probs_in, pl->rnn_in, pl->rnn_critic_in, pl->value_preds, pl->actions, pl->action_log_probs,
                          pl->rnn_states, pl->rnn_states_critic};
    for (const void* q : f32s)
        if (!aligned(q, 4)) return fail("misaligned pointer: float32 arrays need 4-byte alignment");
    if (!aligned(pl->actions_in, pl->actions_int64 ? 8 : 4)) return fail("misaligned pointer: actions_in needs the alignment of its type");
    // every used array: a slot is at least as long as the rows it receives, so slots t and t + 1 do not overlap
    if (((rnn || rnnc) && pl->stride_dones < L) || (pl->values && pl->stride_value_preds < L) || (pl->actions_in && pl->stride_actions < L * k) ||
        (pl->log_probs_in && pl->stride_action_log_probs < L * k) || (rnn && pl->stride_rnn_states < L * row) ||
        (rnnc && pl->stride_rnn_states_critic < L * rowc))
        return fail("misaligned or overlapping strides: every stride must be at least one slot (lanes x row elements)");
    const int64_t blocks = (L + LI_LANES - 1) / LI_LANES;
    if (blocks > 0x7fffffffLL) return fail("too many lanes for one launch");
    if (!pl->values && !pl->actions_in && !pl->log_probs_in && !rnn && !rnnc) return GMPE_OK;
    LiArgs a{};
    const int64_t t = pl->t;
    a.lanes = L; a.k = (int32_t)k; a.a64 = pl->actions_int64;
    a.done = (rnn || rnnc) ? pl->dones + t * pl->stride_dones : nullptr;
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
    GMPE_HIP_CHECK(hipSetDevice(device));
    hipLaunchKernelGGL(k_insert_learner, dim3((unsigned)blocks), dim3(LI_BLOCK), 0, static_cast<hipStream_t>(stream), a);
    GMPE_HIP_CHECK(hipGetLastError());
    return GMPE_OK;
}
