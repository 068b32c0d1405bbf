// gmpe_infos.hip — what run()'s log and eval intervals compute from device data (include/gmpe.h gmpe_env_infos / gmpe_eval_step / gmpe_eval_mean):
// Runner.process_infos + log_env (onpolicy/runner/shared/base_runner.py:194-302) as the per-agent means over envs of the 18 info columns, and the
// bookkeeping of GMPERunner.eval (graph_mpe_runner.py:445-516): reward sums, per-env masks, the zeroed RNN rows and the scalar mean of the sums.
// Handle-less: the arrays are all it needs. No atomics, no allocation, no workspace, no host synchronisation, capturable.
//
// k_chunked_mean<CT>: float64 NumPy's np.mean of a contiguous list, bit for bit, for CT columns per workgroup. NumPy's add.reduce hands the N values
// to its inner loop in consecutive chunks of 8192 (the reduce buffer), starts from +0.0, and adds each chunk's pairwise_sum in order; pairwise_sum
// splits a chunk at n2 = n/2 - (n/2) % 8 until a piece has at most 128 values, which is np_sum's leaf (gmpe_np_sum.h). Per chunk:
//   * thread 0 writes the chunk's split tree to LDS as a post-order program (leaf l / add) with the leaves' (offset, size) — once per chunk size, so
//     twice at the most (the full chunks and the last one);
//   * the leaves are evaluated in parallel: thread (l, c) sums leaf l of column c, c fastest, so the 256 lanes read BLOCK / CT rows of CT consecutive
//     floats each (info rows are 18 floats: a tile of 32 columns is 128 contiguous bytes of one env's A * 18);
//   * one thread per column runs the program over the leaf sums in LDS with an LDS value stack: exactly the recursion's adds;
//   * the column's accumulator takes the chunk sum; after the last chunk it is divided by N.
// k_eval_step: one workgroup per ES_ENVS envs, as gmpe_eval.hip's record kernels: the env threads find whether all agents are done, then the whole
// workgroup writes sums, masks and the zeroed RNN rows of its envs as flat loops over their contiguous ranges.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "gmpe_host.h"          // include/gmpe.h, the error text, GMPE_HIP_CHECK
#include "gmpe_np_sum.h"        // np_sum: NumPy's pairwise_sum for n <= 128

#pragma clang fp contract(off)

namespace {

constexpr int K = GMPE_INFO_KEYS;
constexpr int I_TTG = 2;                       // config.INFO_KEYS: Time_req_to_goal
constexpr int CM_BLOCK = 256;
constexpr int CHUNK = GMPE_INFOS_CHUNK;        // NumPy's reduce buffer, in elements
constexpr int LEAF = GMPE_INFOS_LEAF;          // pairwise_sum's PW_BLOCKSIZE
constexpr int MAX_LEAVES = CHUNK / (LEAF / 2); // a split piece above LEAF has halves above LEAF / 2 - 4: fewer than 128 leaves + slack
constexpr int MAX_TOKENS = 2 * MAX_LEAVES;
constexpr int MAX_DEPTH = 16;                  // 8192 -> 128 is 6 splits; the uneven splits of other sizes add at most one
constexpr int INFO_CT = 32, MEAN_CT = 1;
constexpr int ES_BLOCK = 256;
constexpr int ES_ENVS = 16;

struct MeanArgs {
    int64_t n;                 // values per column
    int64_t stride;            // elements between consecutive values of a column
    int cols;                  // columns, consecutive in memory
    double* out;               // [cols]
};

struct InfoLoad {              // info f32 [N, A, K]; Time_req_to_goal == -1 -> T * dt (base_runner.py:215-216)
    const float* info;
    double tdt;
    __device__ __forceinline__ double operator()(int64_t idx, bool ttg) const {
        const double v = (double)info[idx];
        return ttg && v == -1.0 ? tdt : v;
    }
};

struct F64Load {
    const double* values;
    __device__ __forceinline__ double operator()(int64_t idx, bool) const { return values[idx]; }
};

// The split tree of pairwise_sum over m values, as a post-order program: tok[i] >= 0 is "push the sum of leaf tok[i]", -1 "add the two on top".
struct Program {
    int n_leaves, n_tokens, overflow;
    int leaf_off[MAX_LEAVES], leaf_n[MAX_LEAVES];
    int16_t tok[MAX_TOKENS];
    int st_off[MAX_DEPTH], st_n[MAX_DEPTH], st_state[MAX_DEPTH];
};

__device__ void build_program(Program& pr, int m) {
    int sp = 0, nl = 0, nt = 0, overflow = 0;
    pr.st_off[0] = 0; pr.st_n[0] = m; pr.st_state[0] = 0; sp = 1;
    while (sp > 0) {
        const int top = sp - 1;
        const int n = pr.st_n[top], off = pr.st_off[top], state = pr.st_state[top];
        const int n2 = n / 2 - (n / 2) % 8;
        if (n <= LEAF) {
            if (nl < MAX_LEAVES && nt < MAX_TOKENS) {
                pr.leaf_off[nl] = off; pr.leaf_n[nl] = n; pr.tok[nt++] = (int16_t)nl; ++nl;
            } else overflow = 1;
            --sp;
        } else if (state == 2) {
            if (nt < MAX_TOKENS) pr.tok[nt++] = -1; else overflow = 1;
            --sp;
        } else if (sp >= MAX_DEPTH) {          // cannot happen for m <= CHUNK; kept so that no index can leave the arrays
            overflow = 1;
            --sp;
        } else {
            pr.st_state[top] = state + 1;
            pr.st_off[sp] = state == 0 ? off : off + n2;
            pr.st_n[sp] = state == 0 ? n2 : n - n2;
            pr.st_state[sp] = 0;
            ++sp;
        }
    }
    pr.n_leaves = nl; pr.n_tokens = nt; pr.overflow = overflow;
}

template <int CT, class Load>
__global__ __launch_bounds__(CM_BLOCK) void k_chunked_mean(MeanArgs p, Load load) {
    __shared__ Program pr;
    __shared__ double leaf_sum[MAX_LEAVES * CT];
    __shared__ double vstack[MAX_DEPTH * CT];
    const int tid = threadIdx.x;
    const int cc = tid % CT, l0 = tid / CT;
    const int c = (int)blockIdx.x * CT + cc;                 // this thread's column
    const bool live = c < p.cols;
    const bool ttg = c % K == I_TTG;
    double acc = 0.0;                                        // add.reduce starts from the identity
    int cur_m = -1;
    bool bad = false;
    for (int64_t base = 0; base < p.n; base += CHUNK) {
        const int m = (int)(p.n - base < CHUNK ? p.n - base : CHUNK);
        if (m != cur_m) {                                    // uniform over the workgroup
            if (tid == 0) build_program(pr, m);
            cur_m = m;
            __syncthreads();
        }
        bad = bad || pr.overflow;
        const int nl = pr.n_leaves;
        if (live)
            for (int l = l0; l < nl; l += CM_BLOCK / CT) {
                const int64_t first = (base + pr.leaf_off[l]) * p.stride + c;
                leaf_sum[l * CT + cc] = np_sum(pr.leaf_n[l], [&](int i) { return load(first + (int64_t)i * p.stride, ttg); });
            }
        __syncthreads();
        if (live && l0 == 0 && !pr.overflow) {
            int sp = 0;
            const int nt = pr.n_tokens;
            for (int i = 0; i < nt; ++i) {
                const int t = pr.tok[i];
                if (t >= 0 ? sp >= MAX_DEPTH : sp < 2) {     // cannot happen for a program of build_program; no index leaves the stack
                    bad = true;
                    break;
                }
                if (t >= 0) {
                    vstack[sp * CT + cc] = leaf_sum[t * CT + cc];
                    ++sp;
                } else {
                    const double r = vstack[(sp - 2) * CT + cc] + vstack[(sp - 1) * CT + cc];
                    vstack[(sp - 2) * CT + cc] = r;
                    --sp;
                }
            }
            acc = acc + vstack[cc];
        }
        __syncthreads();                                     // the next chunk overwrites leaf_sum, and perhaps the program
    }
    if (live && l0 == 0) p.out[c] = bad ? __longlong_as_double(0x7ff8000000000000ll) : acc / (double)p.n;
}

struct StepArgs {
    int N, A, first;
    uint32_t row;              // floats of one agent's RNN state, 0 without rnn
    const float* reward;
    const uint8_t* done;
    double* sums;
    float* masks;
    float* rnn;
};

__global__ __launch_bounds__(ES_BLOCK) void k_eval_step(StepArgs p) {
    __shared__ uint8_t all_sh[ES_ENVS];
    const int A = p.A, tid = threadIdx.x;
    const int64_t env0 = (int64_t)blockIdx.x * ES_ENVS;
    const int ne = (int)(p.N - env0 < ES_ENVS ? p.N - env0 : ES_ENVS);
    if (tid < ne) {
        const uint8_t* d = p.done + (env0 + tid) * A;
        bool all = true;
        for (int a = 0; a < A; ++a) all = all && d[a] != 0;
        all_sh[tid] = all;
    }
    __syncthreads();
    const int lanes = ne * A;
    const int64_t lane0 = env0 * A;
    for (int i = tid; i < lanes; i += ES_BLOCK) {
        const double r = (double)p.reward[lane0 + i];
        p.sums[lane0 + i] = (p.first ? 0.0 : p.sums[lane0 + i]) + r;        // np.sum(axis=0): one add per step, in step order, from +0.0
        p.masks[lane0 + i] = all_sh[i / A] ? 0.0f : 1.0f;
    }
    if (!p.rnn) return;
    const uint32_t per = (uint32_t)A * p.row;                // <= 64 * 2^20 floats per env
    for (int w = 0; w < ne; ++w) {
        if (!all_sh[w]) continue;                            // uniform over the workgroup
        float* rs = p.rnn + (env0 + w) * (int64_t)per;
        for (uint32_t i = tid; i < per; i += ES_BLOCK) rs[i] = 0.0f;
    }
}

bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

int fail(const char* fn, const std::string& m) { return gmpe::report_error(GMPE_ERR_INVALID_ARG, std::string(fn) + ": " + m); }

}  // namespace

extern "C" {

int gmpe_env_infos(int device, const gmpe_env_infos_plan* pl, void* stream) {
    const char* fn = "gmpe_env_infos";
    if (!pl) return fail(fn, "null plan");
    if (pl->num_envs < 1) return fail(fn, "num_envs must be >= 1");
    if (pl->num_agents < 1 || pl->num_agents > GMPE_MAX_AGENTS) return fail(fn, "num_agents must be in 1 .. 64");
    if (pl->episode_length < 1) return fail(fn, "episode_length must be >= 1");
    if (pl->reserved != 0) return fail(fn, "reserved must be 0");
    if (!isfinite(pl->dt)) return fail(fn, "dt must be finite");
    if (!pl->info) return fail(fn, "info is null");
    if (!pl->out) return fail(fn, "out is null");
    if (!aligned(pl->info, 4)) return fail(fn, "info must be 4-byte aligned");
    if (!aligned(pl->out, 8)) return fail(fn, "out must be 8-byte aligned");
    const int cols = pl->num_agents * K;
    MeanArgs a{pl->num_envs, cols, cols, pl->out};
    InfoLoad load{pl->info, (double)pl->episode_length * pl->dt};
    GMPE_HIP_CHECK(hipSetDevice(device));
    hipLaunchKernelGGL((k_chunked_mean<INFO_CT, InfoLoad>), dim3((unsigned)((cols + INFO_CT - 1) / INFO_CT)), dim3(CM_BLOCK), 0,
                       static_cast<hipStream_t>(stream), a, load);
    GMPE_HIP_CHECK(hipGetLastError());
    return GMPE_OK;
}

int gmpe_eval_step(int device, const gmpe_eval_step_plan* pl, void* stream) {
    const char* fn = "gmpe_eval_step";
    if (!pl) return fail(fn, "null plan");
    if (pl->num_envs < 1) return fail(fn, "num_envs must be >= 1");
    if (pl->num_agents < 1 || pl->num_agents > GMPE_MAX_AGENTS) return fail(fn, "num_agents must be in 1 .. 64");
    if (pl->first != 0 && pl->first != 1) return fail(fn, "first must be 0 or 1");
    if (pl->rnn_states && (pl->rnn_row < 1 || pl->rnn_row > (1 << 20))) return fail(fn, "rnn_row must be in 1 .. 2^20 with rnn_states");
    if (!pl->rnn_states && pl->rnn_row != 0) return fail(fn, "rnn_row must be 0 without rnn_states");
    if (!pl->reward) return fail(fn, "reward is null");
    if (!pl->done) return fail(fn, "done is null");
    if (!pl->sums) return fail(fn, "sums is null");
    if (!pl->masks) return fail(fn, "masks is null");
    if (!aligned(pl->reward, 4)) return fail(fn, "reward must be 4-byte aligned");
    if (!aligned(pl->sums, 8)) return fail(fn, "sums must be 8-byte aligned");
    if (!aligned(pl->masks, 4)) return fail(fn, "masks must be 4-byte aligned");
    if (!aligned(pl->rnn_states, 4)) return fail(fn, "rnn_states must be 4-byte aligned");
    StepArgs a{pl->num_envs, pl->num_agents, pl->first, pl->rnn_states ? (uint32_t)pl->rnn_row : 0u, pl->reward, pl->done, pl->sums, pl->masks,
               pl->rnn_states};
    GMPE_HIP_CHECK(hipSetDevice(device));
    hipLaunchKernelGGL(k_eval_step, dim3((unsigned)(((int64_t)pl->num_envs + ES_ENVS - 1) / ES_ENVS)), dim3(ES_BLOCK), 0,
                       static_cast<hipStream_t>(stream), a);
    GMPE_HIP_CHECK(hipGetLastError());
    return GMPE_OK;
}

int gmpe_eval_mean(int device, const gmpe_eval_mean_plan* pl, void* stream) {
    const char* fn = "gmpe_eval_mean";
    if (!pl) return fail(fn, "null plan");
    if (pl->count < 1 || pl->count > ((int64_t)1 << 40)) return fail(fn, "count must be in 1 .. 2^40");
    if (!pl->values) return fail(fn, "values is null");
    if (!pl->out) return fail(fn, "out is null");
    if (!aligned(pl->values, 8)) return fail(fn, "values must be 8-byte aligned");
    if (!aligned(pl->out, 8)) return fail(fn, "out must be 8-byte aligned");
    MeanArgs a{pl->count, 1, 1, pl->out};
    F64Load load{pl->values};
    GMPE_HIP_CHECK(hipSetDevice(device));
    hipLaunchKernelGGL((k_chunked_mean<MEAN_CT, F64Load>), dim3(1), dim3(CM_BLOCK), 0, static_cast<hipStream_t>(stream), a, load);
    GMPE_HIP_CHECK(hipGetLastError());
    return GMPE_OK;
}

}  // extern "C"
