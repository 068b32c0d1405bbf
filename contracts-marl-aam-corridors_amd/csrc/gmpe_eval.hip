// gmpe_eval.hip — evaluation of a policy over a batch of episodes (include/gmpe.h gmpe_episode_record / gmpe_episode_record_series /
// gmpe_episode_metrics / gmpe_episode_summary): GMPERunner.render(get_metrics=True) (onpolicy/runner/shared/graph_mpe_runner.py:526-1060) with one
// episode per env, or R episodes per env played back to back across the engine's auto-resets.
// Handle-less: the record state and the step outputs are all it needs. No atomics in global memory, no allocation, no host synchronisation, capturable.
//
// k_episode_record, k_episode_record_series: one workgroup per ER_ENVS envs. Threads 0 .. ER_ENVS-1 own one env each: they read its dones (record_head:
// every agent's mask to LDS) and rewards and do the entry's own bookkeeping: one episode adds the rewards to `ret` while the env is live and copies its
// info rows once when it finishes; the series advances the env's (episode, t_in_ep, ret). Then the whole workgroup writes the masks,
// available_actions and the zeroed RNN rows of its envs as flat loops over their contiguous ranges (record_tail). Head and tail are one piece of
// code; the bookkeeping is two, each measured the better on one workload.
// k_episode_metrics: one thread per env for the columns; A extra workgroups each reduce one agent's Dists_traveled / ttg over the N envs (each
// thread a fixed strided subset in order, then a fixed LDS tree).
// k_episode_summary: one workgroup per column. The ranks the order statistics need are selected exactly by an 8-pass radix selection on the
// order-preserving u64 keys of the f64 values (LDS histograms of integer counts: their result does not depend on the order of the adds).
// Parity: `#pragma clang fp contract(off)`; sums over agents follow NumPy's pairwise_sum (n < 8: sequential; else 8 accumulators, their tree,
// then the tail), so the columns equal float64 NumPy on the same f32 info rows.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "gmpe_host.h"          // include/gmpe.h, the error text, GMPE_HIP_CHECK
#include "gmpe_np_sum.h"        // np_sum: NumPy's pairwise_sum for n <= 128

#pragma clang fp contract(off)

namespace {

constexpr int K = GMPE_EVAL_INFO_WIDTH;
constexpr int M = GMPE_EVAL_NUM_COLUMNS;
constexpr int ER_BLOCK = 256;
constexpr int ER_ENVS = 16;        // envs per record workgroup: 256 workgroups at 4096 envs; masks / rows of the block are contiguous ranges
constexpr int EM_BLOCK = 256;
constexpr int ES_BLOCK = 256;
constexpr int ES_RANKS = 8;        // min, p10 floor / next, median pair, p90 floor / next, max

// info columns (config.INFO_KEYS)
enum { I_DIST_TO_GOAL = 1, I_TTG = 2, I_AGENT_COLL = 3, I_OBST_COLL = 4, I_DIST_MEAN = 5, I_DIST_VAR = 6, I_MEAN_BY_VAR = 7, I_DISTS_TRAV = 8,
       I_TIME_MEAN = 10, I_TIME_STDDEV = 11, I_TIME_MEAN_BY_STDDEV = 12, I_CONFORMANCE = 13, I_DELTA_SPACING = 14, I_SPACING_VIOL = 15 };

// what both record kernels read and write alike
struct StepArgs {
    int N, A, T, n_act, rnn_row;
    const float* reward;
    const uint8_t* done;
    const float* info;
    float* final_info;
    float* masks;
    float* avail;
    float* rnn;
};

// The head of a record kernel, for the thread that owns env n (slot tid of its workgroup): its dones to done_sh, every agent's mask to mask_sh;
// returns whether all its agents are done.
__device__ __forceinline__ bool record_head(const StepArgs& p, int64_t n, int tid, uint8_t* done_sh, uint8_t* mask_sh) {
    const int A = p.A;
    const uint8_t* d = p.done + n * A;
    bool all = true;
    for (int a = 0; a < A; ++a) {
        const uint8_t v = d[a] != 0;
        done_sh[tid * A + a] = v;
        all = all && v;
    }
    for (int a = 0; a < A; ++a) mask_sh[tid * A + a] = all || !done_sh[tid * A + a];     // dones_env rows: all ones
    return all;
}

// The tail of a record kernel, by the whole workgroup after the barrier: the masks, the stop rows of available_actions and the zeroed RNN rows of its
// ne envs from env0 on, as flat loops over their contiguous ranges.
__device__ __forceinline__ void record_tail(const StepArgs& p, int64_t env0, int ne, int tid, const uint8_t* done_sh, const uint8_t* mask_sh) {
    const int lanes = ne * p.A;
    const int64_t lane0 = env0 * p.A;
    for (int i = tid; i < lanes; i += ER_BLOCK) p.masks[lane0 + i] = mask_sh[i] ? 1.0f : 0.0f;
    // 32-bit index math: a workgroup's ranges are below 2^32 elements (n_actions <= 4096, rnn_row <= 2^20)
    const uint32_t na = (uint32_t)p.n_act, stop = na / 2;
    const uint32_t nav = (uint32_t)lanes * na;
    float* av = p.avail + lane0 * na;
    for (uint32_t i = tid; i < nav; i += ER_BLOCK) {
        const uint32_t lane = i / na, j = i - lane * na;
        av[i] = (mask_sh[lane] || j == stop) ? 1.0f : 0.0f;
    }
    if (!p.rnn) return;
    const uint32_t row = (uint32_t)p.rnn_row, nr = (uint32_t)lanes * row;
    float* rs = p.rnn + lane0 * row;
    for (uint32_t i = tid; i < nr; i += ER_BLOCK)
        if (done_sh[i / row]) rs[i] = 0.0f;
}

struct RecArgs {
    StepArgs s;
    int t;
    uint8_t* live;
    int32_t* steps;
    double* ret;
};

__global__ __launch_bounds__(ER_BLOCK) void k_episode_record(RecArgs p) {
    __shared__ uint8_t mask_sh[ER_ENVS * GMPE_MAX_AGENTS];
    __shared__ uint8_t done_sh[ER_ENVS * GMPE_MAX_AGENTS];
    const int A = p.s.A;
    const int64_t env0 = (int64_t)blockIdx.x * ER_ENVS;
    const int ne = (int)(p.s.N - env0 < ER_ENVS ? p.s.N - env0 : ER_ENVS);
    const int tid = threadIdx.x;
    if (tid < ne) {
        const int64_t n = env0 + tid;
        const bool all = record_head(p.s, n, tid, done_sh, mask_sh);
        if (p.live[n]) {
            const float* r = p.s.reward + n * A;
            double* acc = p.ret + n * A;
            for (int a = 0; a < A; ++a) acc[a] = acc[a] + (double)r[a];
            if (all || p.t == p.s.T - 1) {
                const float* s = p.s.info + n * A * K;
                float* o = p.s.final_info + n * A * K;
                for (int i = 0; i < A * K; ++i) o[i] = s[i];
                p.steps[n] = p.t + 1;
                p.live[n] = 0;
            }
        }
    }
    __syncthreads();
    record_tail(p.s, env0, ne, tid, done_sh, mask_sh);
}

// The record for R episodes per env played back to back across the engine's auto-resets. The env threads advance their env's own (episode, t_in_ep, ret)
// state, write the episode's length and returns when it ends at this step and leave the episode index in LDS (-1: no end); the whole workgroup copies the
// info rows of the envs that ended an episode into row e * N + n of final_info.
// Offsets into the [R, N, ...] arrays are 64-bit: R * N * A * 18 passes 2^31 at sizes the summary accepts.
struct SeriesArgs {
    StepArgs s;
    int R;
    int32_t* episode;
    int32_t* t_in_ep;
    double* ret;
    int32_t* steps;
    double* ret_out;
};

__global__ __launch_bounds__(ER_BLOCK) void k_episode_record_series(SeriesArgs p) {
    __shared__ uint8_t mask_sh[ER_ENVS * GMPE_MAX_AGENTS];
    __shared__ uint8_t done_sh[ER_ENVS * GMPE_MAX_AGENTS];
    __shared__ int32_t end_sh[ER_ENVS];                       // the episode index an env ends at this step, or -1
    const int A = p.s.A;
    const int64_t env0 = (int64_t)blockIdx.x * ER_ENVS;
    const int ne = (int)(p.s.N - env0 < ER_ENVS ? p.s.N - env0 : ER_ENVS);
    const int tid = threadIdx.x;
    if (tid < ne) {
        const int64_t n = env0 + tid;
        const bool all = record_head(p.s, n, tid, done_sh, mask_sh);
        int32_t ended = -1;
        const int32_t e = p.episode[n];
        if (e < p.R) {
            const float* r = p.s.reward + n * A;
            double* acc = p.ret + n * A;
            const int32_t t = p.t_in_ep[n] + 1;
            if (all || t == p.s.T) {
                const int64_t row = (int64_t)e * p.s.N + n;
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
    // the info rows of the envs that ended an episode: A * K contiguous floats per env, to row e * N + n. The branch is uniform over the
    // workgroup, so a step at which no env of the block ends costs ER_ENVS LDS reads here.
    const int per = A * K;
    for (int w = 0; w < ne; ++w) {
        const int32_t e = end_sh[w];
        if (e < 0) continue;
        const float* src = p.s.info + (env0 + w) * per;
        float* dst = p.s.final_info + ((int64_t)e * p.s.N + env0 + w) * per;
        for (int i = tid; i < per; i += ER_BLOCK) dst[i] = src[i];
    }
    record_tail(p.s, env0, ne, tid, done_sh, mask_sh);
}

struct MetArgs {
    int N, A, T, row_blocks;
    double tdt, thresh;            // T * dt (the reference's `episode_length * self.dt`), min_dist_thresh
    const int32_t* steps;
    const double* ret;
    const float* fi;
    double* out;
    double* dists;
    double* times;
};

__device__ __forceinline__ double ttg(const float* row, double tdt) {
    const double v = (double)row[I_TTG];
    return v == -1.0 ? tdt : v;
}

__global__ __launch_bounds__(EM_BLOCK) void k_episode_metrics(MetArgs p) {
    const int A = p.A;
    if ((int)blockIdx.x < p.row_blocks) {
        const int64_t n = (int64_t)blockIdx.x * EM_BLOCK + threadIdx.x;
        if (n >= p.N) return;
        const float* fi = p.fi + n * A * K;
        const double* r = p.ret + n * A;
        auto at = [&](int a, int k) { return (double)fi[a * K + k]; };
        double* o = p.out + n * M;
        o[GMPE_EVAL_REWARD] = np_sum(A, [&](int a) { return r[a]; }) / A;
        double fmax = ttg(fi, p.tdt) / p.tdt;
        for (int a = 1; a < A; ++a) fmax = fmax >= ttg(fi + a * K, p.tdt) / p.tdt || fmax != fmax ? fmax : ttg(fi + a * K, p.tdt) / p.tdt;
        o[GMPE_EVAL_FRAC] = fmax;
        int succ = 0;
        for (int a = 0; a < A; ++a) succ += at(a, I_DIST_TO_GOAL) < p.thresh;
        o[GMPE_EVAL_SUCCESS] = (double)succ / A;
        double coll = 0.0;
        for (int a = 0; a < A; ++a) {
            coll = coll + at(a, I_AGENT_COLL) / 2.0;
            coll = coll + at(a, I_OBST_COLL);
        }
        o[GMPE_EVAL_COLLISIONS] = coll;
        const int l = A - 1;
        o[GMPE_EVAL_FAIRNESS] = at(l, I_MEAN_BY_VAR);
        o[GMPE_EVAL_DIST_MEAN] = at(l, I_DIST_MEAN);
        o[GMPE_EVAL_TIME_MEAN] = at(l, I_TIME_MEAN);
        o[GMPE_EVAL_TIME_FAIRNESS] = at(l, I_TIME_MEAN_BY_STDDEV);
        o[GMPE_EVAL_STDDEV_PARAM] = 1.0 / (at(l, I_DIST_VAR) + 0.0001);
        o[GMPE_EVAL_TIME_STDDEV_PARAM] = 1.0 / (at(l, I_TIME_STDDEV) + 0.0001);
        o[GMPE_EVAL_TOTAL_DISTS] = np_sum(A, [&](int a) { return at(a, I_DISTS_TRAV); });
        o[GMPE_EVAL_TOTAL_TIME] = np_sum(A, [&](int a) { return ttg(fi + a * K, p.tdt); });
        o[GMPE_EVAL_CONFORMANCE] = np_sum(A, [&](int a) { return at(a, I_CONFORMANCE); }) / A;
        o[GMPE_EVAL_DELTA_SPACE] = np_sum(A, [&](int a) { return at(a, I_DELTA_SPACING); }) / A;
        o[GMPE_EVAL_SPACING_VIOLATIONS] = np_sum(A, [&](int a) { return at(a, I_SPACING_VIOL); }) / A;
        o[GMPE_EVAL_STEPS] = (double)p.steps[n];
        return;
    }
    // per-agent sums over the episodes: a fixed strided order per thread, then a fixed tree
    __shared__ double sd[EM_BLOCK], st[EM_BLOCK];
    const int a = (int)blockIdx.x - p.row_blocks;
    double s0 = 0.0, s1 = 0.0;
    for (int64_t n = threadIdx.x; n < p.N; n += EM_BLOCK) {
        const float* row = p.fi + (n * A + a) * K;
        s0 += (double)row[I_DISTS_TRAV];
        s1 += ttg(row, p.tdt);
    }
    sd[threadIdx.x] = s0;
    st[threadIdx.x] = s1;
    __syncthreads();
    for (int h = EM_BLOCK / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            sd[threadIdx.x] = sd[threadIdx.x] + sd[threadIdx.x + h];
            st[threadIdx.x] = st[threadIdx.x] + st[threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        p.dists[a] = sd[0];
        p.times[a] = st[0];
    }
}

// order-preserving key of a double (non-NaN): ascending u64 order == ascending value order (-0.0 sorts before +0.0)
__device__ __forceinline__ uint64_t key_of(double x) {
    const uint64_t b = (uint64_t)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double value_of(uint64_t k) {
    const uint64_t b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}

// NumPy's _lerp (numpy/lib/_function_base_impl.py)
__device__ __forceinline__ double np_lerp(double a, double b, double t) {
    const double diff = b - a;
    return t >= 0.5 ? b - diff * (1.0 - t) : a + diff * t;
}

struct PctIdx { int64_t lo, hi; double g; };

// np.percentile(x, q), method 'linear': virtual index (n - 1) * (q / 100), previous = floor, next = previous + 1, both n - 1 at or past the end
__device__ __forceinline__ PctIdx pct_index(int64_t n, double q) {
    const double v = (double)(n - 1) * (q / 100.0);
    PctIdx r;
    if (v >= (double)(n - 1)) {
        r.lo = r.hi = n - 1;
    } else {
        r.lo = (int64_t)floor(v);
        r.hi = r.lo + 1;
    }
    r.g = v - floor(v);
    return r;
}

struct SumArgs {
    int64_t n;
    int cols, succ_col, succ_a;
    const double* table;
    double* out;
};

__global__ __launch_bounds__(ES_BLOCK) void k_episode_summary(SumArgs p) {
    __shared__ uint32_t hist[ES_RANKS][256];
    __shared__ double red[ES_BLOCK];
    __shared__ uint64_t prefix[ES_RANKS];
    __shared__ int64_t rank_left[ES_RANKS];
    __shared__ int nan_sh;
    const int c = blockIdx.x, tid = threadIdx.x;
    const int64_t n = p.n;
    const int C = p.cols;
    const double* col = p.table + c;
    double* o = p.out + (int64_t)c * GMPE_EVAL_NUM_STATS;
    const PctIdx q10 = pct_index(n, 10.0), q90 = pct_index(n, 90.0);
    const int64_t mid_lo = (n % 2) ? n / 2 : n / 2 - 1, mid_hi = n / 2;

    // mean: a fixed strided order per thread, a fixed tree
    auto block_sum = [&](double s) {
        red[tid] = s;
        __syncthreads();
        for (int h = ES_BLOCK / 2; h > 0; h >>= 1) {
            if (tid < h) red[tid] = red[tid] + red[tid + h];
            __syncthreads();
        }
        const double r = red[0];
        __syncthreads();
        return r;
    };

    if (c == p.succ_col) {
        // the flattened [n, A] 0/1 matrix: S ones, the rest zeros; np.min / percentile / max over it, mean S / (n*A)
        double s = 0.0;
        for (int64_t i = tid; i < n; i += ES_BLOCK) s += rint(col[i * C] * p.succ_a);
        const double S = block_sum(s);
        if (tid != 0) return;
        const int64_t total = n * p.succ_a, zeros = total - (int64_t)S;
        auto at = [&](int64_t r) { return r >= zeros ? 1.0 : 0.0; };
        const PctIdx f10 = pct_index(total, 10.0), f90 = pct_index(total, 90.0);
        const int64_t flo = (total % 2) ? total / 2 : total / 2 - 1, fhi = total / 2;
        const double mean = S / (double)total;
        o[GMPE_EVAL_STAT_MIN] = at(0);
        o[GMPE_EVAL_STAT_P10] = np_lerp(at(f10.lo), at(f10.hi), f10.g);
        o[GMPE_EVAL_STAT_MEDIAN] = (total % 2) ? at(fhi) : (at(flo) + at(fhi)) / 2.0;
        o[GMPE_EVAL_STAT_P90] = np_lerp(at(f90.lo), at(f90.hi), f90.g);
        o[GMPE_EVAL_STAT_MAX] = at(total - 1);
        o[GMPE_EVAL_STAT_MEAN] = mean;
        o[GMPE_EVAL_STAT_STD] = sqrt(((double)zeros * (mean * mean) + S * ((1.0 - mean) * (1.0 - mean))) / (double)total);
        return;
    }

    double s = 0.0;
    int nan_local = 0;
    for (int64_t i = tid; i < n; i += ES_BLOCK) {
        const double x = col[i * C];
        s += x;
        nan_local |= x != x;
    }
    if (tid == 0) nan_sh = 0;
    const double mean = block_sum(s) / (double)n;
    if (nan_local) nan_sh = 1;                      // every writer stores the same value
    double v = 0.0;
    for (int64_t i = tid; i < n; i += ES_BLOCK) {
        const double d = col[i * C] - mean;
        v += d * d;
    }
    const double var = block_sum(v) / (double)n;   // also orders nan_sh's stores before the read below
    if (tid == 0) {
        o[GMPE_EVAL_STAT_MEAN] = mean;
        o[GMPE_EVAL_STAT_STD] = sqrt(var);
    }
    if (nan_sh) {
        if (tid == 0) {
            const double q = __longlong_as_double(0x7ff8000000000000ll);
            o[GMPE_EVAL_STAT_MIN] = o[GMPE_EVAL_STAT_P10] = o[GMPE_EVAL_STAT_MEDIAN] = o[GMPE_EVAL_STAT_P90] = o[GMPE_EVAL_STAT_MAX] = q;
        }
        return;
    }

    // exact radix selection of the 8 ranks, one byte per pass from the top
    if (tid < ES_RANKS) {
        const int64_t ranks[ES_RANKS] = {0, q10.lo, q10.hi, mid_lo, mid_hi, q90.lo, q90.hi, n - 1};
        prefix[tid] = 0;
        rank_left[tid] = ranks[tid];
    }
    for (int shift = 56; shift >= 0; shift -= 8) {
        for (int i = tid; i < ES_RANKS * 256; i += ES_BLOCK) (&hist[0][0])[i] = 0;
        __syncthreads();
        const uint64_t hmask = shift == 56 ? 0ull : (~0ull << (shift + 8));
        uint64_t pf[ES_RANKS];
#pragma unroll
        for (int j = 0; j < ES_RANKS; ++j) pf[j] = prefix[j];
        for (int64_t i = tid; i < n; i += ES_BLOCK) {
            const uint64_t k = key_of(col[i * C]);
            const uint32_t b = (uint32_t)(k >> shift) & 255u;
#pragma unroll
            for (int j = 0; j < ES_RANKS; ++j)
                if ((k & hmask) == pf[j]) atomicAdd(&hist[j][b], 1u);
        }
        __syncthreads();
        if (tid < ES_RANKS) {
            int64_t r = rank_left[tid];
            uint32_t b = 0;
            for (; b < 255; ++b) {
                if (r < (int64_t)hist[tid][b]) break;
                r -= hist[tid][b];
            }
            rank_left[tid] = r;
            prefix[tid] = prefix[tid] | ((uint64_t)b << shift);
        }
        __syncthreads();
    }
    if (tid == 0) {
        double x[ES_RANKS];
#pragma unroll
        for (int j = 0; j < ES_RANKS; ++j) x[j] = value_of(prefix[j]);
        o[GMPE_EVAL_STAT_MIN] = x[0];
        o[GMPE_EVAL_STAT_P10] = np_lerp(x[1], x[2], q10.g);
        o[GMPE_EVAL_STAT_MEDIAN] = (n % 2) ? x[4] : (x[3] + x[4]) / 2.0;
        o[GMPE_EVAL_STAT_P90] = np_lerp(x[5], x[6], q90.g);
        o[GMPE_EVAL_STAT_MAX] = x[7];
    }
}

bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

int fail(const char* fn, const std::string& m) { return gmpe::report_error(GMPE_ERR_INVALID_ARG, std::string(fn) + ": " + m); }

// The checks the two record entry points make alike, in the order both make them. `dims`, `missing`, `a4` and `mis8` are the entry point's own findings:
// its steps and further dimensions (a message, or null), whether a required pointer is null, its 4-byte arrays' addresses or-ed together, and its 8-byte arrays
// (a message, or null), reported at their place in that order.
template <class Plan>
int check_record_plan(const char* fn, const Plan* pl, const char* dims, bool missing, uintptr_t a4, const char* mis8) {
    if (pl->num_envs < 1 || pl->num_agents < 1 || pl->num_agents > GMPE_MAX_AGENTS) return fail(fn, "need num_envs >= 1 and 1 <= num_agents <= 64");
    if (dims) return fail(fn, dims);
    if (pl->n_actions < 1 || pl->n_actions > 4096) return fail(fn, "n_actions must be in 1 .. 4096");
    if (pl->rnn_states && (pl->rnn_row < 1 || pl->rnn_row > (1 << 20))) return fail(fn, "rnn_row must be in 1 .. 2^20 with rnn_states");
    if (missing) return fail(fn, "null pointer: only rnn_states may be NULL");
    if (a4 & 3) return fail(fn, "misaligned pointer: 4-byte arrays need 4-byte alignment");
    if (mis8) return fail(fn, mis8);
    const int64_t lanes = (int64_t)pl->num_envs * pl->num_agents;
    if (lanes * pl->n_actions > (int64_t)1 << 40 || (pl->rnn_states && lanes * pl->rnn_row > (int64_t)1 << 40)) return fail(fn, "arrays too large");
    return GMPE_OK;
}

template <class Plan>
StepArgs step_args(const Plan* pl) {
    return StepArgs{pl->num_envs, pl->num_agents, pl->num_steps, pl->n_actions, pl->rnn_states ? pl->rnn_row : 0, pl->reward, pl->done, pl->info,
                    pl->final_info, pl->masks, pl->available_actions, pl->rnn_states};
}

unsigned record_blocks(int num_envs) { return (unsigned)(((int64_t)num_envs + ER_ENVS - 1) / ER_ENVS); }

}  // namespace

extern "C" {

int gmpe_episode_record(int device, const gmpe_episode_record_plan* pl, void* stream) {
    const char* fn = "gmpe_episode_record";
    if (!pl) return fail(fn, "null plan");
    const bool missing = !pl->reward || !pl->done || !pl->info || !pl->live || !pl->steps || !pl->ret || !pl->final_info || !pl->masks || !pl->available_actions;
    const uintptr_t a4 = (uintptr_t)pl->reward | (uintptr_t)pl->info | (uintptr_t)pl->steps | (uintptr_t)pl->final_info | (uintptr_t)pl->masks |
                         (uintptr_t)pl->available_actions | (uintptr_t)pl->rnn_states;
    if (int rc = check_record_plan(fn, pl, pl->num_steps < 1 || pl->t < 0 || pl->t >= pl->num_steps ? "need num_steps >= 1 and 0 <= t < num_steps" : nullptr, missing, a4,
                                   aligned(pl->ret, 8) ? nullptr : "misaligned pointer: ret needs 8-byte alignment"))
        return rc;
    RecArgs a{step_args(pl), pl->t, pl->live, pl->steps, pl->ret};
    GMPE_HIP_CHECK(hipSetDevice(device));
    hipLaunchKernelGGL(k_episode_record, dim3(record_blocks(pl->num_envs)), dim3(ER_BLOCK), 0, static_cast<hipStream_t>(stream), a);
    GMPE_HIP_CHECK(hipGetLastError());
    return GMPE_OK;
}

int gmpe_episode_record_series(int device, const gmpe_episode_series_plan* pl, void* stream) {
    const char* fn = "gmpe_episode_record_series";
    if (!pl) return fail(fn, "null plan");
    const char* dims = nullptr;
    if (pl->num_steps < 1) dims = "need num_steps >= 1";
    else if (pl->num_episodes < 1) dims = "need num_episodes >= 1";
    else if ((int64_t)pl->num_episodes * pl->num_envs > 0x7fffffffLL) dims = "num_episodes * num_envs must be at most 2^31 - 1";
    const bool missing = !pl->reward || !pl->done || !pl->info || !pl->episode || !pl->t_in_ep || !pl->ret || !pl->steps || !pl->ret_out || !pl->final_info ||
                         !pl->masks || !pl->available_actions;
    const uintptr_t a4 = (uintptr_t)pl->reward | (uintptr_t)pl->info | (uintptr_t)pl->episode | (uintptr_t)pl->t_in_ep | (uintptr_t)pl->steps |
                         (uintptr_t)pl->final_info | (uintptr_t)pl->masks | (uintptr_t)pl->available_actions | (uintptr_t)pl->rnn_states;
    if (int rc = check_record_plan(fn, pl, dims, missing, a4, aligned(pl->ret, 8) && aligned(pl->ret_out, 8) ? nullptr
                                   : "misaligned pointer: ret and ret_out need 8-byte alignment"))
        return rc;
    SeriesArgs a{step_args(pl), pl->num_episodes, pl->episode, pl->t_in_ep, pl->ret, pl->steps, pl->ret_out};
    GMPE_HIP_CHECK(hipSetDevice(device));
    hipLaunchKernelGGL(k_episode_record_series, dim3(record_blocks(pl->num_envs)), dim3(ER_BLOCK), 0, static_cast<hipStream_t>(stream), a);
    GMPE_HIP_CHECK(hipGetLastError());
    return GMPE_OK;
}

int gmpe_episode_metrics(int device, const gmpe_episode_metrics_plan* pl, void* stream) {
    const char* fn = "gmpe_episode_metrics";
    if (!pl) return fail(fn, "null plan");
    if (pl->num_envs < 1 || pl->num_agents < 1 || pl->num_agents > GMPE_MAX_AGENTS) return fail(fn, "need num_envs >= 1 and 1 <= num_agents <= 64");
    if (pl->num_steps < 1 || pl->reserved != 0) return fail(fn, "need num_steps >= 1 and reserved 0");
    if (!(pl->dt > 0.0) || !isfinite(pl->dt) || pl->min_dist_thresh != pl->min_dist_thresh) return fail(fn, "dt must be finite and > 0, min_dist_thresh a number");
    if (!pl->steps || !pl->ret || !pl->final_info || !pl->episodes) return fail(fn, "null pointer: only dists_traveled / time_taken may be NULL");
    if ((pl->dists_traveled == nullptr) != (pl->time_taken == nullptr)) return fail(fn, "dists_traveled and time_taken are given together or not at all");
    if (!aligned(pl->steps, 4) || !aligned(pl->final_info, 4) || !aligned(pl->ret, 8) || !aligned(pl->episodes, 8) || !aligned(pl->dists_traveled, 8) ||
        !aligned(pl->time_taken, 8))
        return fail(fn, "misaligned pointer");
    const bool sums = pl->dists_traveled != nullptr;
    const int row_blocks = (pl->num_envs + EM_BLOCK - 1) / EM_BLOCK;
    MetArgs a{pl->num_envs, pl->num_agents, pl->num_steps, row_blocks, (double)pl->num_steps * pl->dt, pl->min_dist_thresh, pl->steps, pl->ret,
              pl->final_info, pl->episodes, pl->dists_traveled, pl->time_taken};
    GMPE_HIP_CHECK(hipSetDevice(device));
    hipLaunchKernelGGL(k_episode_metrics, dim3((unsigned)(row_blocks + (sums ? pl->num_agents : 0))), dim3(EM_BLOCK), 0,
                       static_cast<hipStream_t>(stream), a);
    GMPE_HIP_CHECK(hipGetLastError());
    return GMPE_OK;
}

int gmpe_episode_summary(int device, const gmpe_episode_summary_plan* pl, void* stream) {
    const char* fn = "gmpe_episode_summary";
    if (!pl) return fail(fn, "null plan");
    if (pl->num_rows < 1 || pl->num_rows > 0x7fffffffLL) return fail(fn, "num_rows must be in 1 .. 2^31 - 1");
    if (pl->num_columns < 1 || pl->num_columns > 64 || pl->reserved != 0) return fail(fn, "num_columns must be in 1 .. 64 and reserved 0");
    if (pl->success_column >= pl->num_columns || pl->success_column < -1) return fail(fn, "success_column must be -1 or a column index");
    if (pl->success_column >= 0 && (pl->success_agents < 1 || pl->success_agents > GMPE_MAX_AGENTS)) return fail(fn, "success_agents must be in 1 .. 64");
    if (!pl->table || !pl->out) return fail(fn, "null pointer");
    if (!aligned(pl->table, 8) || !aligned(pl->out, 8)) return fail(fn, "misaligned pointer: f64 arrays need 8-byte alignment");
    SumArgs a{pl->num_rows, pl->num_columns, pl->success_column, pl->success_agents, pl->table, pl->out};
    GMPE_HIP_CHECK(hipSetDevice(device));
    hipLaunchKernelGGL(k_episode_summary, dim3((unsigned)pl->num_columns), dim3(ES_BLOCK), 0, static_cast<hipStream_t>(stream), a);
    GMPE_HIP_CHECK(hipGetLastError());
    return GMPE_OK;
}

}  // extern "C"
