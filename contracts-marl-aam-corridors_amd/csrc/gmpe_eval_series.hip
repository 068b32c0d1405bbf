// gmpe_eval_series.hip — gmpe_episode_record_series (include/gmpe.h): the per-step record of gmpe_eval.hip's k_episode_record for R episodes per env
// played back to back across the engine's auto-resets. Handle-less; no atomics, no allocation, no host synchronisation, capturable.
//
// k_episode_record_series keeps k_episode_record's shape: one workgroup per ES_ENVS envs. Threads 0 .. ES_ENVS-1 own one env each: they read its
// dones and rewards, advance its own (episode, t_in_ep, ret) state, write the episode's length and returns when it ends at this step and leave the
// episode index in LDS (-1: no end). Then the whole workgroup writes the masks, available_actions and the zeroed RNN rows of its envs as flat
// loops over their contiguous ranges, and copies the info rows of the envs that ended an episode into row e * N + n of final_info.
// Offsets into the [R, N, ...] arrays are 64-bit: R * N * A * 18 passes 2^31 at sizes the summary accepts.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "gmpe_host.h"          // include/gmpe.h, the error text, GMPE_HIP_CHECK

#pragma clang fp contract(off)

namespace {

constexpr int K = GMPE_EVAL_INFO_WIDTH;
constexpr int ES_BLOCK = 256;
constexpr int ES_ENVS = 16;        // envs per workgroup, as k_episode_record: the masks / rows of the block are contiguous ranges

struct SeriesArgs {
    int N, A, T, R, n_act, rnn_row;
    const float* reward;
    const uint8_t* done;
    const float* info;
    int32_t* episode;
    int32_t* t_in_ep;
    double* ret;
    int32_t* steps;
    double* ret_out;
    float* final_info;
    float* masks;
    float* avail;
    float* rnn;
};

__global__ __launch_bounds__(ES_BLOCK) void k_episode_record_series(SeriesArgs p) {
    __shared__ uint8_t mask_sh[ES_ENVS * GMPE_MAX_AGENTS];
    __shared__ uint8_t done_sh[ES_ENVS * GMPE_MAX_AGENTS];
    __shared__ int32_t end_sh[ES_ENVS];                       // the episode index an env ends at this step, or -1
    const int A = p.A;
    const int64_t env0 = (int64_t)blockIdx.x * ES_ENVS;
    const int ne = (int)(p.N - env0 < ES_ENVS ? p.N - env0 : ES_ENVS);
    const int tid = threadIdx.x;
    if (tid < ne) {
        const int64_t n = env0 + tid;
        const uint8_t* d = p.done + n * A;
        bool all = true;
        for (int a = 0; a < A; ++a) {
            const uint8_t v = d[a] != 0;
            done_sh[tid * A + a] = v;
            all = all && v;
        }
        for (int a = 0; a < A; ++a) mask_sh[tid * A + a] = all || !done_sh[tid * A + a];     // dones_env rows: all ones
        int32_t ended = -1;
        const int32_t e = p.episode[n];
        if (e < p.R) {
            const float* r = p.reward + n * A;
            double* acc = p.ret + n * A;
            const int32_t t = p.t_in_ep[n] + 1;
            if (all || t == p.T) {
                const int64_t row = (int64_t)e * p.N + n;
                double* o = p.ret_out + row * A;
                for (int a = 0; a < A; ++a) {
                    o[a] = acc[a] + (double)r[a];
                    acc[a] = 0.0;
                }
                p.steps[row] = t;
                p.episode[n] = e + 1;
                p.t_in_ep[n] = 0;
                ended = e;
            } else {
                for (int a = 0; a < A; ++a) acc[a] = acc[a] + (double)r[a];
                p.t_in_ep[n] = t;
            }
        }
        end_sh[tid] = ended;
    }
    __syncthreads();
    const int lanes = ne * A;
    const int64_t lane0 = env0 * A;
    for (int i = tid; i < lanes; i += ES_BLOCK) p.masks[lane0 + i] = mask_sh[i] ? 1.0f : 0.0f;
    // 32-bit index math: a workgroup's ranges are below 2^32 elements (n_actions <= 4096, rnn_row <= 2^20)
    const uint32_t na = (uint32_t)p.n_act, stop = na / 2;
    const uint32_t nav = (uint32_t)lanes * na;
    float* av = p.avail + lane0 * na;
    for (uint32_t i = tid; i < nav; i += ES_BLOCK) {
        const uint32_t lane = i / na, j = i - lane * na;
        av[i] = (mask_sh[lane] || j == stop) ? 1.0f : 0.0f;
    }
    // the info rows of the envs that ended an episode: A * K contiguous floats per env, to row e * N + n. The branch is uniform over the
    // workgroup, so a step at which no env of the block ends costs ES_ENVS LDS reads here.
    const int per = A * K;
    for (int w = 0; w < ne; ++w) {
        const int32_t e = end_sh[w];
        if (e < 0) continue;
        const float* src = p.info + (env0 + w) * per;
        float* dst = p.final_info + ((int64_t)e * p.N + env0 + w) * per;
        for (int i = tid; i < per; i += ES_BLOCK) dst[i] = src[i];
    }
    if (!p.rnn) return;
    const uint32_t row = (uint32_t)p.rnn_row, nr = (uint32_t)lanes * row;
    float* rs = p.rnn + lane0 * row;
    for (uint32_t i = tid; i < nr; i += ES_BLOCK)
        if (done_sh[i / row]) rs[i] = 0.0f;
}

bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

int fail(const char* fn, const std::string& m) { return gmpe::report_error(GMPE_ERR_INVALID_ARG, std::string(fn) + ": " + m); }

}  // namespace

extern "C" int gmpe_episode_record_series(int device, const gmpe_episode_series_plan* pl, void* stream) {
    const char* fn = "gmpe_episode_record_series";
    if (!pl) return fail(fn, "null plan");
    if (pl->num_envs < 1 || pl->num_agents < 1 || pl->num_agents > GMPE_MAX_AGENTS) return fail(fn, "need num_envs >= 1 and 1 <= num_agents <= 64");
    if (pl->num_steps < 1) return fail(fn, "need num_steps >= 1");
    if (pl->num_episodes < 1) return fail(fn, "need num_episodes >= 1");
    if ((int64_t)pl->num_episodes * pl->num_envs > 0x7fffffffLL) return fail(fn, "num_episodes * num_envs must be at most 2^31 - 1");
    if (pl->n_actions < 1 || pl->n_actions > 4096) return fail(fn, "n_actions must be in 1 .. 4096");
    if (pl->rnn_states && (pl->rnn_row < 1 || pl->rnn_row > (1 << 20))) return fail(fn, "rnn_row must be in 1 .. 2^20 with rnn_states");
    if (!pl->reward || !pl->done || !pl->info || !pl->episode || !pl->t_in_ep || !pl->ret || !pl->steps || !pl->ret_out || !pl->final_info ||
        !pl->masks || !pl->available_actions)
        return fail(fn, "null pointer: only rnn_states may be NULL");
    const void* f4[] = {pl->reward, pl->info, pl->episode, pl->t_in_ep, pl->steps, pl->final_info, pl->masks, pl->available_actions, pl->rnn_states};
    for (const void* q : f4)
        if (!aligned(q, 4)) return fail(fn, "misaligned pointer: 4-byte arrays need 4-byte alignment");
    if (!aligned(pl->ret, 8) || !aligned(pl->ret_out, 8)) return fail(fn, "misaligned pointer: ret and ret_out need 8-byte alignment");
    const int64_t lanes = (int64_t)pl->num_envs * pl->num_agents;
    if (lanes * pl->n_actions > (int64_t)1 << 40 || (pl->rnn_states && lanes * pl->rnn_row > (int64_t)1 << 40)) return fail(fn, "arrays too large");
    SeriesArgs a{pl->num_envs, pl->num_agents, pl->num_steps, pl->num_episodes, pl->n_actions, pl->rnn_states ? pl->rnn_row : 0, pl->reward, pl->done,
                 pl->info, pl->episode, pl->t_in_ep, pl->ret, pl->steps, pl->ret_out, pl->final_info, pl->masks, pl->available_actions, pl->rnn_states};
    const int64_t blocks = ((int64_t)pl->num_envs + ES_ENVS - 1) / ES_ENVS;
    GMPE_HIP_CHECK(hipSetDevice(device));
    hipLaunchKernelGGL(k_episode_record_series, dim3((unsigned)blocks), dim3(ES_BLOCK), 0, static_cast<hipStream_t>(stream), a);
    GMPE_HIP_CHECK(hipGetLastError());
    return GMPE_OK;
}
