// gmpe_mb_edges.hip — the edge list of a PPO minibatch straight from the adjacency a rollout stores (include/gmpe.h gmpe_minibatch_edges): what
// TransformerConvNet.process_adj (onpolicy/algorithms/utils/gnn_new.py:329-358) makes of the adj_batch of one minibatch, without writing that [rows, E, E] tensor.
// Handle-less, like the gather.
//
// Count, scan, write — the scheme of k_edge_count / k_edge_scan / k_edge_write (gmpe_step.hip) behind the minibatch row map (gmpe_mb_map.h, the gather's own):
//   k_mbe_count: a wave per graph, four graphs per workgroup. The wave decodes its graph's (t, n, a) once (wave-uniform: the graph index goes through
//                readfirstlane, so the permutation entry is a scalar load), lanes run over the entries; per-graph count and per-workgroup total.
//   k_mbe_scan:  one workgroup, the per-workgroup totals in fixed chunks of 1024 with a running carry -> exclusive offsets in place, total -> n_edges (saturating).
//   k_mbe_write: the same walk; ballot / popcount compaction with a wave-uniform running base, so edges land in (graph, row, col) order.
// Sources: a matrix ([T+1, N, A, E, E] or compact [T+1, N, E, E]; 16-byte loads when E*E % 4 == 0 and the pointers allow) or the f64 entity table, whose entries
// are rebuilt with gmpe_expand.h under the engine's -ffp-contract=off flags: the bits k_adj_from_table and k_mb_table give.
// No atomics, no allocation, no host synchronisation; all sums are integers, so the result does not depend on the launch geometry.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "gmpe_host.h"          // include/gmpe.h, the error text, GMPE_HIP_CHECK
#include "gmpe_expand.h"
#include "gmpe_mb_map.h"

#pragma clang fp contract(off)

namespace {

constexpr int MBE_BLOCK = 256, MBE_WAVES = 4, MBE_SCAN = 1024;

struct MbeArgs {
    const int64_t* perm;     // NULL: identity
    int64_t offset;
    uint32_t T, N, A, L;
    uint32_t chunks;         // chunks of this minibatch (recurrent)
    uint32_t n_valid;        // valid permutation entries
    int32_t mode;
    uint32_t graphs;
    const char* src;
    int64_t slot_stride;     // bytes
    uint32_t row_bytes;      // bytes of one source row: E*E*4 (matrices), W*8 (table)
    int32_t per_agent;       // matrix source: 1 = [.., N, A, E, E]
    int32_t E, W;
    float d;
    int32_t inclusive;
    long long* boff;         // [workgroups] totals, then exclusive offsets
    int32_t* counts;         // [graphs]
    void* edge_index;
    float* edge_attr;
    long long cap;
    int32_t* n_edges;
    uint32_t nblocks;
};

__device__ __forceinline__ bool edge_pred(float v, float d, int inclusive) {
    return (inclusive ? v <= d : v < d) && v > 0.0f;
}

// Source row of graph g (wave-uniform), NULL for an out-of-range permutation entry: nothing of it is read.
__device__ __forceinline__ const char* graph_src(const MbeArgs& p, uint32_t g) {
    const gmpe::Sample sm = p.perm ? gmpe::sample_of<false>(p, g, false) : gmpe::sample_of<true>(p, g, false);
    if (!sm.ok) return nullptr;
    const size_t row = p.per_agent ? (size_t)sm.n * p.A + sm.a : (size_t)sm.n;
    return p.src + (int64_t)sm.t * p.slot_stride + row * p.row_bytes;
}

// VEC consecutive entries from entry q of one graph. TABLE: rebuilt from the entity table; else loaded (one 16-byte load with VEC = 4).
template <bool TABLE, int VEC>
__device__ __forceinline__ void load_entries(const MbeArgs& p, const char* s, int q, bool in, float (&v)[VEC]) {
    if (TABLE) {
        const int E = p.E, qq = in ? q : 0, r = qq / E, c = qq - r * E;
        v[0] = gmpe::adj_entry_from_table(reinterpret_cast<const double*>(s), E, p.W, r, c);
    } else if (VEC == 4) {
        const float4 x = in ? *reinterpret_cast<const float4*>(s + (size_t)q * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    } else {
        v[0] = in ? *reinterpret_cast<const float*>(s + (size_t)q * 4) : 0.0f;
    }
}

template <bool TABLE, int VEC> struct Unroll { static constexpr int U = TABLE ? 2 : (VEC == 4 ? 4 : 8); };   // loads in flight per lane

template <bool TABLE, int VEC>
__global__ __launch_bounds__(MBE_BLOCK) void k_mbe_count(MbeArgs p) {
    constexpr int U = Unroll<TABLE, VEC>::U;
    __shared__ int wc[MBE_WAVES];
    const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const uint32_t g = blockIdx.x * MBE_WAVES + w;
    int c = 0;
    if (g < p.graphs) {
        const char* s = graph_src(p, g);
        if (s) {
            const int EE = p.E * p.E;
            for (int q0 = 0; q0 < EE; q0 += 64 * VEC * U) {
                float v[U][VEC];
#pragma unroll
                for (int u = 0; u < U; ++u) { const int q = q0 + (u * 64 + (int)lane) * VEC; load_entries<TABLE, VEC>(p, s, q, q < EE, v[u]); }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const bool in = q0 + (u * 64 + (int)lane) * VEC < EE;
#pragma unroll
                    for (int k = 0; k < VEC; ++k) c += (int)__popcll(__ballot(in && edge_pred(v[u][k], p.d, p.inclusive)));
                }
            }
        }
        if (lane == 0) p.counts[g] = c;
    }
    if (lane == 0) wc[w] = c;
    __syncthreads();
    if (threadIdx.x == 0) p.boff[blockIdx.x] = (long long)wc[0] + wc[1] + wc[2] + wc[3];
}

// Exclusive scan of the per-workgroup totals, in place; chunks of MBE_SCAN in order with a running carry. One workgroup.
__global__ __launch_bounds__(MBE_SCAN) void k_mbe_scan(long long* __restrict__ boff, uint32_t nb, int32_t* __restrict__ n_edges) {
    __shared__ long long wtot[MBE_SCAN / 64];
    __shared__ long long carry;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (t == 0) carry = 0;
    __syncthreads();
    for (uint32_t first = 0; first < nb; first += MBE_SCAN) {
        const uint32_t b = first + t;
        const long long c = b < nb ? boff[b] : 0;
        long long incl = c;
        for (int o = 1; o < 64; o <<= 1) { const long long x = __shfl_up(incl, o, 64); if (lane >= o) incl += x; }
        if (lane == 63) wtot[w] = incl;
        __syncthreads();
        long long pre = carry;
        for (int k = 0; k < w; ++k) pre += wtot[k];
        if (b < nb) boff[b] = pre + incl - c;
        __syncthreads();
        if (t == MBE_SCAN - 1) carry = pre + incl;
        __syncthreads();
    }
    if (t == 0) *n_edges = carry > 0x7fffffffLL ? 0x7fffffff : (int32_t)carry;
}

template <bool TABLE, int VEC, bool I64>
__global__ __launch_bounds__(MBE_BLOCK) void k_mbe_write(MbeArgs p) {
    constexpr int U = Unroll<TABLE, VEC>::U;
    const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const uint32_t g = blockIdx.x * MBE_WAVES + w;
    if (g >= p.graphs) return;
    if (p.counts[g] <= 0) return;                              // also every graph of an out-of-range entry
    long long run = p.boff[blockIdx.x];                        // wave-uniform running position
    for (uint32_t k = 0; k < w; ++k) run += p.counts[blockIdx.x * MBE_WAVES + k];
    if ((unsigned long long)run >= (unsigned long long)p.cap) return;
    const char* s = graph_src(p, g);
    if (!s) return;
    const int E = p.E, EE = E * E;
    const long long id0 = (long long)g * E, cap = p.cap;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int q0 = 0; q0 < EE; q0 += 64 * VEC * U) {
        float v[U][VEC];
#pragma unroll
        for (int u = 0; u < U; ++u) { const int q = q0 + (u * 64 + (int)lane) * VEC; load_entries<TABLE, VEC>(p, s, q, q < EE, v[u]); }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int q = q0 + (u * 64 + (int)lane) * VEC;
            const bool in = q < EE;
            bool f[VEC];
            int pre = 0, tot = 0;
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                f[k] = in && edge_pred(v[u][k], p.d, p.inclusive);
                const unsigned long long bal = __ballot(f[k]);
                pre += (int)__popcll(bal & below);             // edges of the lanes before this one
                tot += (int)__popcll(bal);
            }
            int mine = 0;
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                if (f[k]) {
                    const long long pos = run + pre + mine;
                    if ((unsigned long long)pos < (unsigned long long)cap) {
                        const int r = (q + k) / E, cc = (q + k) - r * E;
                        if (I64) { static_cast<long long*>(p.edge_index)[pos] = id0 + r; static_cast<long long*>(p.edge_index)[cap + pos] = id0 + cc; }
                        else { static_cast<int32_t*>(p.edge_index)[pos] = (int32_t)(id0 + r); static_cast<int32_t*>(p.edge_index)[cap + pos] = (int32_t)(id0 + cc); }
                        p.edge_attr[pos] = v[u][k];
                    }
                    ++mine;
                }
            }
            run += tot;
        }
    }
}

int fail(int code, const std::string& m) { return gmpe::report_error(code, m); }

size_t ws_bytes(int64_t graphs) {
    const int64_t nb = (graphs + MBE_WAVES - 1) / MBE_WAVES;
    return (size_t)((nb * 8 + graphs * 4 + 15) / 16 * 16);
}

}  // namespace

extern "C" {

int gmpe_minibatch_edges_workspace_bytes(int64_t graphs, size_t* bytes_out) {
    if (!bytes_out || graphs < 1 || graphs > 0x7fffffffLL)
        return fail(GMPE_ERR_INVALID_ARG, "gmpe_minibatch_edges_workspace_bytes: need 1 <= graphs < 2^31 and an output");
    *bytes_out = ws_bytes(graphs);
    return GMPE_OK;
}

int gmpe_minibatch_edges(const gmpe_config* cfg, int device, const gmpe_mb_edges_plan* pl, void* stream) {
    const char* me = "gmpe_minibatch_edges: ";
    auto bad = [&](const std::string& m) { return fail(GMPE_ERR_INVALID_ARG, me + m); };
    if (!pl) return bad("null plan");
    if (pl->mode != GMPE_MB_FEED_FORWARD && pl->mode != GMPE_MB_RECURRENT) return bad("unknown mode");
    if (pl->source < GMPE_MBE_ADJ || pl->source > GMPE_MBE_TABLE) return bad("unknown source");
    if (pl->reserved != 0) return bad("reserved must be 0");
    const bool rec = pl->mode == GMPE_MB_RECURRENT, table = pl->source == GMPE_MBE_TABLE;
    if (pl->T < 1 || pl->N < 1 || pl->A < 1 || (rec && pl->L < 1)) return bad("need T, N, A >= 1 (and L >= 1 recurrent)");
    const int64_t samples = (int64_t)pl->T * pl->N * pl->A;
    if (samples > 0x7fffffffLL) return bad("T * N * A must be below 2^31");
    if (pl->E < 1 || pl->E > GMPE_MAX_ENTITIES) return bad("E must be 1 .. GMPE_MAX_ENTITIES");
    if (!(pl->max_edge_dist == pl->max_edge_dist)) return bad("max_edge_dist is NaN");
    if (pl->rows < 1 || pl->offset < 0) return bad("need rows >= 1 and offset >= 0");
    if (pl->perm) {
        if (pl->perm_len < 1 || pl->offset + pl->rows > pl->perm_len) return bad("need 0 <= offset <= offset + rows <= perm_len");
        if (((uintptr_t)pl->perm & 7) != 0) return bad("the permutation must be 8-byte aligned int64");
    } else if (pl->offset + pl->rows > 0x7fffffffLL) {
        return bad("offset + rows must be below 2^31 with the identity permutation");
    }
    const int64_t graphs = rec ? pl->rows * pl->L : pl->rows;
    if (graphs > 0x7fffffffLL) return bad("too many graphs in one minibatch");
    if (!pl->index64 && graphs * pl->E > 0x7fffffffLL) return bad("node ids overflow int32 (use index64)");
    int W = 0;
    if (table) {
        if (!cfg) return bad("the table source needs a config");
        if (cfg->abi_version != GMPE_ABI_VERSION) return bad("gmpe_config.abi_version mismatch");
        W = gmpe_entity_table_width(cfg);
        if (cfg->num_agents != pl->A || cfg->num_agents > GMPE_MAX_AGENTS || cfg->num_landmarks < cfg->num_agents || gmpe_num_entities(cfg) != pl->E)
            return bad("the table source needs a config whose agents and entities are the plan's A and E");
    }
    const int64_t EE4 = (int64_t)pl->E * pl->E * 4;
    const int64_t row_bytes = table ? (int64_t)W * 8 : EE4;
    const int64_t slot = row_bytes * (pl->source == GMPE_MBE_ADJ ? (int64_t)pl->N * pl->A : (int64_t)pl->N);
    if (!pl->src) return bad("null src");
    if (pl->slot_stride < slot) return bad("slot_stride is smaller than one slot of the source");
    if ((((uintptr_t)pl->src | (uintptr_t)pl->slot_stride) & (table ? 7 : 3)) != 0)
        return bad("src and slot_stride must be 4-byte aligned (8-byte for the table source)");
    if (!pl->n_edges || ((uintptr_t)pl->n_edges & 3)) return bad("n_edges must be a 4-byte aligned device pointer");
    if (!pl->workspace || ((uintptr_t)pl->workspace & 7)) return bad("the workspace must be an 8-byte aligned device pointer");
    if (pl->workspace_bytes < ws_bytes(graphs)) return bad("the workspace is smaller than gmpe_minibatch_edges_workspace_bytes(graphs)");
    if (pl->cap < 0) return bad("cap must be >= 0");
    const bool write = pl->edge_index != nullptr;
    if (write) {
        if (!pl->edge_attr || ((uintptr_t)pl->edge_attr & 3)) return bad("edge_attr must be a 4-byte aligned device pointer when edge_index is given");
        if ((uintptr_t)pl->edge_index & (pl->index64 ? 7 : 3)) return bad("edge_index must be aligned to its element size");
    } else if (pl->reuse_counts) {
        return bad("reuse_counts needs edge_index (there is nothing else to do)");
    }
    MbeArgs a;
    a.perm = pl->perm; a.offset = pl->offset;
    a.T = pl->T; a.N = pl->N; a.A = pl->A; a.L = rec ? pl->L : 1;
    a.chunks = (uint32_t)pl->rows;
    a.n_valid = (uint32_t)(rec ? samples / pl->L : samples);
    a.mode = pl->mode; a.graphs = (uint32_t)graphs;
    a.src = static_cast<const char*>(pl->src); a.slot_stride = pl->slot_stride; a.row_bytes = (uint32_t)row_bytes;
    a.per_agent = pl->source == GMPE_MBE_ADJ; a.E = pl->E; a.W = W;
    a.d = pl->max_edge_dist; a.inclusive = pl->inclusive != 0;
    a.nblocks = (uint32_t)((graphs + MBE_WAVES - 1) / MBE_WAVES);
    a.boff = static_cast<long long*>(pl->workspace);
    a.counts = reinterpret_cast<int32_t*>(a.boff + a.nblocks);
    a.edge_index = pl->edge_index; a.edge_attr = pl->edge_attr; a.cap = pl->cap; a.n_edges = pl->n_edges;
    const bool vec4 = !table && (EE4 & 15) == 0 && (((uintptr_t)pl->src | (uintptr_t)pl->slot_stride) & 15) == 0;
    GMPE_HIP_CHECK(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(a.nblocks), block(MBE_BLOCK);
    if (!pl->reuse_counts) {
        if (table) hipLaunchKernelGGL((k_mbe_count<true, 1>), grid, block, 0, st, a);
        else if (vec4) hipLaunchKernelGGL((k_mbe_count<false, 4>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_mbe_count<false, 1>), grid, block, 0, st, a);
        GMPE_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_mbe_scan, dim3(1), dim3(MBE_SCAN), 0, st, a.boff, a.nblocks, a.n_edges);
        GMPE_HIP_CHECK(hipGetLastError());
    }
    if (write && pl->cap > 0) {
        const int which = (table ? 4 : (vec4 ? 2 : 0)) + (pl->index64 ? 1 : 0);
        switch (which) {
        case 0: hipLaunchKernelGGL((k_mbe_write<false, 1, false>), grid, block, 0, st, a); break;
        case 1: hipLaunchKernelGGL((k_mbe_write<false, 1, true>), grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL((k_mbe_write<false, 4, false>), grid, block, 0, st, a); break;
        case 3: hipLaunchKernelGGL((k_mbe_write<false, 4, true>), grid, block, 0, st, a); break;
        case 4: hipLaunchKernelGGL((k_mbe_write<true, 1, false>), grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL((k_mbe_write<true, 1, true>), grid, block, 0, st, a); break;
        }
        GMPE_HIP_CHECK(hipGetLastError());
    }
    return GMPE_OK;
}

}  // extern "C"
