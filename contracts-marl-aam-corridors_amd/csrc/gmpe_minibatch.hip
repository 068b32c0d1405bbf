// gmpe_minibatch.hip — PPO minibatches gathered from a rollout on the device (include/gmpe.h gmpe_minibatch_gather): the rows that
// GraphReplayBuffer.feed_forward_generator / recurrent_generator (onpolicy/utils/graph_buffer.py:368-758) index out of the buffer's arrays, for every field of one
// minibatch, without materialising the per-agent arrays the reference indexes. Handle-less: a learner rank may own no envs.
//
// k_mb_copy: one work list over (field, output row, 16 / 8 / 4-byte unit). The host gives every field a contiguous range of workgroups, so a workgroup belongs to
// one field and its field lookup is uniform (scalar loads from the kernel arguments). Each thread decodes its row's sample (t, n, a) from the permutation and copies
// one unit: exact bytes, coalesced stores.
// k_mb_table: the table kinds — node rows and adjacency entries rebuilt from the f64 entity table with gmpe_expand.h, the arithmetic gmpe_expand_node_obs /
// gmpe_expand_adj (and so the engine) use; this TU is compiled with the same -ffp-contract=off, so the bits are the engine's.
// Plain stores: a minibatch (~31 MB at c3) is read by the policy right after, and the Infinity Cache can hold it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "gmpe_host.h"          // include/gmpe.h, the error text, GMPE_HIP_CHECK
#include "gmpe_expand.h"
#include "gmpe_mb_map.h"

#pragma clang fp contract(off)

namespace {

constexpr int MB_BLOCK = 256;

struct MbField {
    const char* src;
    char* dst;
    int64_t slot_stride;
    uint32_t row_bytes;      // output row
    uint32_t src_row;        // source row bytes (the output row's except for the table kinds: W * 8)
    uint32_t units;          // copy: units per row; table: threads per row
    uint32_t total;          // threads of the field: output rows * units
    uint32_t block0;         // first workgroup of the field
    int32_t kind;
    int32_t shift;           // copy: log2 of the unit bytes (4, 3 or 2)
};

struct MbArgs {
    const int64_t* perm;
    int64_t offset;
    uint32_t T, N, A, L;
    uint32_t chunks;         // chunks of this minibatch (recurrent)
    uint32_t n_valid;        // valid permutation entries: T*N*A (feed-forward) or T*N*A / L chunks (recurrent)
    int32_t mode, nf;
    int32_t E, W, Lm, two;   // table kinds: entities, table width, landmarks, two_phase_graph
    MbField f[GMPE_MB_MAX_FIELDS];
};

// Sample (t, n, a) of output row r: gmpe_mb_map.h, shared with the edge lists (gmpe_mb_edges.hip)
using gmpe::Sample;
using gmpe::sample_of;

__device__ __forceinline__ int field_of(const MbArgs& p) {
    int f = 0;
    for (int i = 1; i < p.nf; ++i)
        if (blockIdx.x >= p.f[i].block0) f = i;
    return f;
}

__global__ __launch_bounds__(MB_BLOCK) void k_mb_copy(MbArgs p) {
    const MbField& F = p.f[field_of(p)];
    const uint32_t u = (blockIdx.x - F.block0) * MB_BLOCK + threadIdx.x;
    if (u >= F.total) return;
    const uint32_t r = u / F.units, q = u - r * F.units;
    const Sample sm = sample_of(p, r, F.kind == GMPE_MB_CHUNK_HEAD);
    if (!sm.ok) return;
    const size_t srow = F.kind == GMPE_MB_ENV_ROW ? (size_t)sm.n : (size_t)sm.n * p.A + sm.a;
    const char* s = F.src + (int64_t)sm.t * F.slot_stride + srow * F.row_bytes + ((size_t)q << F.shift);
    char* d = F.dst + (size_t)r * F.row_bytes + ((size_t)q << F.shift);
    if (F.shift == 4) *reinterpret_cast<uint4*>(d) = *reinterpret_cast<const uint4*>(s);
    else if (F.shift == 3) *reinterpret_cast<uint2*>(d) = *reinterpret_cast<const uint2*>(s);
    else *reinterpret_cast<uint32_t*>(d) = *reinterpret_cast<const uint32_t*>(s);
}

// Table kinds. Node rows: one thread per (output row, entity k), F floats each. Adjacency: one thread per (output row, VEC consecutive entries).
template <int KIND, int VEC>
__global__ __launch_bounds__(MB_BLOCK) void k_mb_table(MbArgs p) {
    const MbField& F = p.f[field_of(p)];
    const uint32_t u = (blockIdx.x - F.block0) * MB_BLOCK + threadIdx.x;
    if (u >= F.total) return;
    const uint32_t r = u / F.units, q = u - r * F.units;
    const Sample sm = sample_of(p, r, false);
    if (!sm.ok) return;
    const double* T = reinterpret_cast<const double*>(F.src + (int64_t)sm.t * F.slot_stride + (size_t)sm.n * F.src_row);
    float* d = reinterpret_cast<float*>(F.dst + (size_t)r * F.row_bytes);
    const int E = p.E;
    if (F.kind == GMPE_MB_TABLE_NODE) {
        gmpe::node_row_from_table<KIND>(T, d + (size_t)q * (KIND == 0 ? 8 : 7), (int)p.A, p.Lm, E, p.W, p.two, (int)sm.a, (int)q);
        return;
    }
    const int e0 = (int)q * VEC;
    float v[VEC];
#pragma unroll
    for (int w = 0; w < VEC; ++w) {
        const int rr = (e0 + w) / E, cc = (e0 + w) - rr * E;
        v[w] = gmpe::adj_entry_from_table(T, E, p.W, rr, cc);
    }
    if (VEC == 4) *reinterpret_cast<float4*>(d + e0) = make_float4(v[0], v[1], v[2], v[3]);
    else d[e0] = v[0];
}

int fail(int code, const std::string& m) { return gmpe::report_error(code, m); }

}  // namespace

extern "C" {

int gmpe_minibatch_gather(const gmpe_config* cfg, int device, const gmpe_minibatch_plan* pl, void* stream) {
    const char* me = "gmpe_minibatch_gather: ";
    auto bad = [&](const std::string& m) { return fail(GMPE_ERR_INVALID_ARG, me + m); };
    if (!pl) return bad("null plan");
    if (pl->mode != GMPE_MB_FEED_FORWARD && pl->mode != GMPE_MB_RECURRENT) return bad("unknown mode");
    if (pl->num_fields < 1 || pl->num_fields > GMPE_MB_MAX_FIELDS) return bad("num_fields must be 1 .. GMPE_MB_MAX_FIELDS");
    const bool rec = pl->mode == GMPE_MB_RECURRENT;
    if (pl->T < 1 || pl->N < 1 || pl->A < 1 || (rec && pl->L < 1)) return bad("need T, N, A >= 1 (and L >= 1 recurrent)");
    const int64_t samples = (int64_t)pl->T * pl->N * pl->A;
    if (samples > 0x7fffffffLL) return bad("T * N * A must be below 2^31");
    if (!pl->perm || pl->perm_len < 1 || pl->offset < 0 || pl->rows < 1 || pl->offset + pl->rows > pl->perm_len)
        return bad("need a permutation, rows >= 1 and 0 <= offset <= offset + rows <= perm_len");
    if (((uintptr_t)pl->perm & 7) != 0) return bad("the permutation must be 8-byte aligned int64");
    const int64_t out_rows = rec ? pl->rows * pl->L : pl->rows;
    if (out_rows > 0x7fffffffLL) return bad("too many rows in one minibatch");
    bool tables = false;
    for (int i = 0; i < pl->num_fields; ++i) tables = tables || pl->fields[i].kind >= GMPE_MB_TABLE_NODE;
    int E = 0, W = 0, Fe = 0, kind = 0;
    if (tables) {
        if (!cfg) return bad("the table kinds need a config");
        if (cfg->abi_version != GMPE_ABI_VERSION) return bad("gmpe_config.abi_version mismatch");
        E = gmpe_num_entities(cfg); W = gmpe_entity_table_width(cfg); Fe = gmpe_node_feats(cfg);
        if (cfg->num_agents != pl->A || cfg->num_agents > GMPE_MAX_AGENTS || cfg->num_landmarks < cfg->num_agents || E > GMPE_MAX_ENTITIES)
            return bad("the table kinds need a config whose agents are the plan's A and whose sizes are in range");
        kind = cfg->graph_feat_type == 1 ? 2 : (cfg->scenario >= GMPE_SCENARIO_ROT_INV ? 1 : 0);
    }
    MbArgs a;
    a.perm = pl->perm; a.offset = pl->offset;
    a.T = pl->T; a.N = pl->N; a.A = pl->A; a.L = rec ? pl->L : 1;
    a.chunks = (uint32_t)pl->rows;
    a.n_valid = (uint32_t)(rec ? samples / pl->L : samples);
    a.mode = pl->mode; a.E = E; a.W = W; a.Lm = cfg ? cfg->num_landmarks : 0; a.two = cfg && cfg->scenario == GMPE_SCENARIO_TWO_PHASE;
    MbArgs b = a;                                     // table fields
    a.nf = b.nf = 0;
    int64_t blocks_a = 0, blocks_b = 0;
    int vec = tables && (E * E) % 4 == 0 ? 4 : 1;    // one instantiation for every table adjacency field
    for (int i = 0; i < pl->num_fields; ++i)
        if (pl->fields[i].kind == GMPE_MB_TABLE_ADJ && ((uintptr_t)pl->fields[i].dst & 15)) vec = 1;
    for (int i = 0; i < pl->num_fields; ++i) {
        const gmpe_mb_field& f = pl->fields[i];
        const std::string at = "field " + std::to_string(i) + ": ";
        if (f.kind < GMPE_MB_ROW || f.kind > GMPE_MB_TABLE_ADJ) return bad(at + "unknown kind");
        if (!f.src || !f.dst) return bad(at + "null src / dst");
        if (f.row_bytes < 4 || (f.row_bytes & 3)) return bad(at + "row_bytes must be a positive multiple of 4");
        if (f.kind == GMPE_MB_CHUNK_HEAD && !rec) return bad(at + "GMPE_MB_CHUNK_HEAD is for the recurrent mode");
        const bool tab = f.kind >= GMPE_MB_TABLE_NODE;
        const int64_t src_row = tab ? (int64_t)W * 8 : f.row_bytes;
        const int64_t slot = src_row * (f.kind == GMPE_MB_ENV_ROW || tab ? pl->N : (int64_t)pl->N * pl->A);
        if (f.slot_stride < slot) return bad(at + "slot_stride is smaller than one slot of the source");
        if (tab && f.row_bytes != (f.kind == GMPE_MB_TABLE_NODE ? E * Fe * 4 : E * E * 4))
            return bad(at + "row_bytes must be E * F * 4 (table node rows) or E * E * 4 (table adjacency) of the config");
        const uintptr_t al = (uintptr_t)f.src | (uintptr_t)f.dst | (uintptr_t)f.slot_stride | (uintptr_t)f.row_bytes;
        if (tab && ((((uintptr_t)f.src | (uintptr_t)f.slot_stride) & 7) || ((uintptr_t)f.dst & 3)))
            return bad(at + "the table must be 8-byte aligned and the output 4-byte aligned");
        if (al & 3) return bad(at + "src, dst and slot_stride must be 4-byte aligned");
        const int64_t rows = f.kind == GMPE_MB_CHUNK_HEAD ? pl->rows : out_rows;
        MbField m;
        m.src = static_cast<const char*>(f.src); m.dst = static_cast<char*>(f.dst);
        m.slot_stride = f.slot_stride; m.row_bytes = (uint32_t)f.row_bytes; m.src_row = (uint32_t)src_row; m.kind = f.kind;
        int64_t units;
        if (!tab) {
            m.shift = (al & 15) == 0 ? 4 : ((al & 7) == 0 ? 3 : 2);
            units = f.row_bytes >> m.shift;
        } else if (f.kind == GMPE_MB_TABLE_NODE) {
            if (kind == 0 && ((uintptr_t)f.dst & 15)) return bad(at + "F = 8 node rows are stored as 16-byte vectors: dst must be 16-byte aligned");
            m.shift = 0;
            units = E;
        } else {
            m.shift = 0;
            units = (int64_t)E * E / vec;
        }
        m.units = (uint32_t)units;
        if (rows * units > 0x7fffffffLL) return bad(at + "too many units in one minibatch");
        m.total = (uint32_t)(rows * units);
        const int64_t nb = (rows * units + MB_BLOCK - 1) / MB_BLOCK;
        MbArgs& dstargs = tab ? b : a;
        int64_t& blocks = tab ? blocks_b : blocks_a;
        m.block0 = (uint32_t)blocks;
        blocks += nb;
        if (blocks > 0x7fffffffLL) return bad("too many workgroups for one launch");
        dstargs.f[dstargs.nf++] = m;
    }
    GMPE_HIP_CHECK(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (a.nf) {
        hipLaunchKernelGGL(k_mb_copy, dim3((unsigned)blocks_a), dim3(MB_BLOCK), 0, st, a);
        GMPE_HIP_CHECK(hipGetLastError());
    }
    if (b.nf) {
        const dim3 grid((unsigned)blocks_b), block(MB_BLOCK);
        switch (kind * 2 + (vec == 4)) {
        case 0: hipLaunchKernelGGL((k_mb_table<0, 1>), grid, block, 0, st, b); break;
        case 1: hipLaunchKernelGGL((k_mb_table<0, 4>), grid, block, 0, st, b); break;
        case 2: hipLaunchKernelGGL((k_mb_table<1, 1>), grid, block, 0, st, b); break;
        case 3: hipLaunchKernelGGL((k_mb_table<1, 4>), grid, block, 0, st, b); break;
        case 4: hipLaunchKernelGGL((k_mb_table<2, 1>), grid, block, 0, st, b); break;
        default: hipLaunchKernelGGL((k_mb_table<2, 4>), grid, block, 0, st, b); break;
        }
        GMPE_HIP_CHECK(hipGetLastError());
    }
    return GMPE_OK;
}

}  // extern "C"
