// gmpe_gnn_wide.hip — the policy's GNNBase forward on graphs of up to 128 nodes (include/gmpe.h gmpe_gnn_forward_wide / gmpe_gnn_forward_wide_table /
// gmpe_gnn_wide_geometry), from both sources: node rows with a dense adjacency, and the fp64 entity table. Forward only: backward's per-graph state at
// 128 nodes is more LDS than a CU has. Up to 64 nodes the entries hand the plan to the narrow entries, whose launch it then is.
//
// Mapping. gmpe_gnn_kernels.h gives a node to a lane of one wave; here it belongs to a thread of a PAIR of waves. A workgroup of 256 threads owns tiles
// of W graphs, W = 2 where two graphs' state (wlay_of, the narrow forward's layout) fits the LDS next to the parameters and 1 above; pair p (waves 2p,
// 2p + 1) owns graph p of the tile and its thread t = 0 .. 127 node t. The pair shares the graph's LDS block. The masked matrix is staged by all
// threads that have the block: the pair's 128 at W = 2, all 256 at W = 1, where the second pair does nothing else. Every loop bound is the same in every
// wave, so every barrier is a uniform workgroup barrier; a pair without a graph computes nothing.
//
// The arithmetic is graph_inputs' and graph_forward<false>'s, statement by statement, with the node's thread in place of the lane, out of the same
// device helpers: a node's sums over its incoming edges run ascending in its own thread and skip what the mask excludes, heads are added ascending, a
// pool adds the nodes ascending in one thread per channel. So a node's chain of operations does not know how many threads the graph has, and a graph of
// <= 64 nodes padded with isolated ones keeps k_gnn_fwd's bits in every original node.
#define GMPE_GNN_WIDE           // gmpe_gnn_table.hip without its entry points: the geometry, gmpe_gnn_kernels.h, and the table plan's checks and binding
#include "gmpe_gnn_table.hip"

namespace {

constexpr int WIDE_MAXE = GMPE_GNN_WIDE_MAX_NODES, PAIR = 2 * 64, NPAIR = BLOCK / PAIR;
static_assert(WIDE_MAXE == PAIR && NPAIR == 2, "a node per thread of a wave pair, two pairs in a workgroup");

// A graph's source (graph_source with the block's staging threads in place of a wave's lanes): the masked matrix into ev by thread s of the ns that have
// the block, and, with `on`, the first F - 1 features of node `node` into its lin1 input row nin -> its type as the float the rows hold.
__device__ __forceinline__ float wide_source(const GnnArgs& p, float* ev, float* nin, int s, int ns, int node, int64_t g, bool on) {
    const int E = p.E, es = E | 1;
    const float* a = p.adj + (g / p.S) * (int64_t)(E * E);
#pragma unroll 1
    for (int f = s; f < E * E; f += ns) {
        const int j = f / E, i = f - j * E;
        const float v = a[f];
        ev[j * es + i] = (v > 0.0f && v < p.maxd) ? v : 0.0f;
    }
    if (!on) return 0.0f;
    const float* xr = p.x + (g * E + node) * p.F;
#pragma unroll 1
    for (int k = 0; k < p.F - 1; ++k) nin[k] = xr[k];
    return xr[p.F - 1];
}
__device__ __forceinline__ float wide_source(const GnnTableArgs& p, float* ev, float* nin, int s, int ns, int node, int64_t g, bool on) {
    const int E = p.E, es = E | 1;
    int64_t idx = !p.tidx ? g / p.tshare : (p.idx64 ? static_cast<const int64_t*>(p.tidx)[g] : (int64_t) static_cast<const int32_t*>(p.tidx)[g]);
    idx = idx < 0 ? 0 : (idx > p.tlast ? p.tlast : idx);
    const double* T = p.tab + idx * p.TW;
#pragma unroll 1
    for (int f = s; f < E * E; f += ns) {
        const int j = f / E, i = f - j * E;
        const float v = gmpe::adj_entry_from_table(T, E, p.TW, j, i);
        ev[j * es + i] = (v > 0.0f && v < p.maxd) ? v : 0.0f;
    }
    if (!on) return 0.0f;
    const int id = p.id[g], ego = id < 0 ? 0 : (id >= p.A ? p.A - 1 : id);
    if (p.kind == 0) gmpe::node_row_from_table<0>(T, nin, p.A, p.NL, E, p.TW, p.two, ego, node);
    else if (p.kind == 1) gmpe::node_row_from_table<1>(T, nin, p.A, p.NL, E, p.TW, p.two, ego, node);
    else gmpe::node_row_from_table<2>(T, nin, p.A, p.NL, E, p.TW, p.two, ego, node);
    return nin[p.F - 1];
}

template <class ARGS>
__global__ __launch_bounds__(BLOCK) void k_gnn_fwd_wide(ARGS p) {
    extern __shared__ __attribute__((aligned(16))) float sh[];
    const int tid = threadIdx.x, E = p.E, es = E | 1, H = p.H;
    const bool two = p.W == NPAIR;
    const int pair = two ? tid / PAIR : 0;              // the graph of the tile whose block this thread stages into
    const int s = two ? tid % PAIR : tid, ns = two ? PAIR : BLOCK;
    const int node = tid % PAIR;
    const bool owner = two || tid < PAIR;               // at W = 1 the second pair stages and waits
    const Lay L = lay_of(p.nemb, p.esz, p.K1, H, p.nconv, p.nel);
    const WLay WL = wlay_of(E, p.nconv, false);
    const float* Wt = sh;
    float* wl = sh + L.np + pair * WL.total;
    const float* ev = wl + WL.ev;
    load_params(p, L, sh, tid);
    __syncthreads();
    const float Hf = (float)H;
    for (int64_t tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
        const int64_t g = tile * p.W + pair;
        const bool active = g < p.rows, on = active && owner && node < E;
        // the graph's inputs: the masked matrix, every node's lin1 input row and its part P of lin1 (graph_inputs)
        {
            float* nin = wl + WL.nin + node * NINS;
            float tf = 0.0f;
            if (active) tf = wide_source(p, wl + WL.ev, nin, s, ns, node, g, on);
            if (on) {
                const int type = tf >= 1.0f ? (tf < (float)p.nemb ? (int)tf : p.nemb - 1) : 0;
                float P[C];
#pragma unroll 1
                for (int k = 0; k < p.esz; ++k) nin[p.F - 1 + k] = Wt[L.emb + type * p.esz + k];
#pragma unroll 1
                for (int k = p.K1 - 1; k < NINS; ++k) nin[k] = 0.0f;
#pragma unroll
                for (int c = 0; c < C; ++c) P[c] = Wt[L.b1 + c];
#pragma unroll 1
                for (int k = 0; k < p.K1 - 1; ++k) {
                    const float v = nin[k];
#pragma unroll
                    for (int c = 0; c < C; ++c) P[c] = fmaf(Wt[L.w1 + c * p.K1 + k], v, P[c]);
                }
                store16(wl + WL.P + node * C, P);
            }
            __syncthreads();
        }
        // the EmbedConv: a node's sum over its incoming edges in double, rounded once
        float x[C];
        double xa[C];
        zero16(xa);
        if (on) {
            float w1e[C];
#pragma unroll
            for (int c = 0; c < C; ++c) w1e[c] = Wt[L.w1 + c * p.K1 + p.K1 - 1];
#pragma unroll 1
            for (int j = 0; j < E; ++j) {
                reload();
                const float e = ev[j * es + node];
                if (e > 0.0f) {
                    float Pj[C], y[C];
                    load16(wl + WL.P + j * C, Pj);
                    edge_forward<false>(p, L, Wt, Pj, w1e, e, y, nullptr);
#pragma unroll
                    for (int c = 0; c < C; ++c) xa[c] += (double)y[c];
                }
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) x[c] = (float)xa[c];
        for (int cc = 0; cc < p.nconv; ++cc) {
            const float* Wc = Wt + L.conv + cc * L.cs;
            float sk[C], o[C];
            zero16(o);
            if (on) lin16(Wc + cws(H), Wc + cbs(H), x, sk);
            for (int h = 0; h < H; ++h) {
                float q[C];
                if (on) {
                    float k[C], v[C];
                    lin16(Wc + cw(H, 0, h), Wc + cb(H, 0, h), x, q);
                    lin16(Wc + cw(H, 1, h), Wc + cb(H, 1, h), x, k);
                    lin16(Wc + cw(H, 2, h), Wc + cb(H, 2, h), x, v);
                    store16(wl + WL.kv + node * 2 * C, k);
                    store16(wl + WL.kv + node * 2 * C + C, v);
                }
                __syncthreads();
                if (on) {
                    float we[C];
                    load16(Wc + cwe(H, h), we);
                    float m = -INFINITY;
#pragma unroll 1
                    for (int j = 0; j < E; ++j) {
                        reload();
                        const float e = ev[j * es + node];
                        if (e > 0.0f) {
                            float k[C];
                            load16(wl + WL.kv + j * 2 * C, k);
                            const float l = edge_logit(q, k, we, e);
                            m = l > m ? l : m;
                        }
                    }
                    float sum = 0.0f, acc[C];
                    zero16(acc);
#pragma unroll 1
                    for (int j = 0; j < E; ++j) {
                        reload();
                        const float e = ev[j * es + node];
                        if (e > 0.0f) {
                            float k[C], v[C];
                            load16(wl + WL.kv + j * 2 * C, k);
                            load16(wl + WL.kv + j * 2 * C + C, v);
                            const float pr = expf(edge_logit(q, k, we, e) - m);
                            sum = sum + pr;
#pragma unroll
                            for (int c = 0; c < C; ++c) acc[c] = fmaf(pr, fmaf(we[c], e, v[c]), acc[c]);
                        }
                    }
                    if (sum > 0.0f) {
#pragma unroll
                        for (int c = 0; c < C; ++c) o[c] = o[c] + __fdiv_rn(acc[c], sum);
                    }
                }
                __syncthreads();                        // the next head's keys and values take this head's place
            }
            if (on) {
#pragma unroll
                for (int c = 0; c < C; ++c) x[c] = activate(p.cact, __fdiv_rn(o[c], Hf) + sk[c]);
            }
        }
        if (on) store16(wl + WL.xs + node * C, x);
        __syncthreads();
        // the gather or the pool: one thread per channel, the nodes ascending
        if (active && owner && node < C) {
            const float* xs = wl + WL.xs;
            float r;
            if (p.aggr == GMPE_GNN_NODE) r = xs[ego_of(p, g) * C + node];
            else {
                r = xs[node];
#pragma unroll 1
                for (int i = 1; i < E; ++i) {
                    reload();
                    const float v = xs[i * C + node];
                    r = p.aggr == GMPE_GNN_MAX ? (v > r ? v : r) : r + v;
                }
                if (p.aggr == GMPE_GNN_MEAN) r = __fdiv_rn(r, (float)E);
            }
            p.out[g * C + node] = r;
        }
        __syncthreads();                                // the next tile overwrites the pairs' state
    }
}

// the wide launch of a checked shape: W graphs side by side, as many as the LDS holds next to the parameters, two at the most
struct WideLayout { int W, nblocks; int64_t ntiles; size_t lds; };
int wide_layout(const char* fn, const gmpe_gnn_plan* pl, const Layout& y, WideLayout& w) {
    const size_t per = (size_t)wlay_of(pl->num_nodes, pl->gnn_layer_n + 1, false).total * sizeof(float), fixed = (size_t)y.L.np * sizeof(float);
    if (fixed + per > (size_t)LDS_CU) return fail(fn, "internal: the LDS layout does not fit");
    w.W = (int)((LDS_CU - fixed) / per);
    w.W = w.W > NPAIR ? NPAIR : w.W;
    w.lds = fixed + w.W * per;
    w.ntiles = (pl->rows + w.W - 1) / w.W;
    w.nblocks = gmpe::resident_grid(w.ntiles, w.lds, 4);
    return GMPE_OK;
}

template <class ARGS>
int launch_wide(int device, const WideLayout& w, ARGS a, int slot, void* stream) {
    a.W = w.W; a.ntiles = w.ntiles;
    GMPE_HIP_CHECK(hipSetDevice(device));
    if (int rc = gmpe::raise_dynamic_lds_once(reinterpret_cast<const void*>(k_gnn_fwd_wide<ARGS>), device, slot, LDS_CU)) return rc;
    GMPE_LAUNCH(k_gnn_fwd_wide<ARGS>, dim3((unsigned)w.nblocks), dim3(BLOCK), w.lds, static_cast<hipStream_t>(stream), a);
    return GMPE_OK;
}

}  // namespace

extern "C" {

int gmpe_gnn_wide_geometry(const gmpe_gnn_plan* plan, int64_t* out) {
    const char* fn = "gmpe_gnn_wide_geometry";
    Layout y = {};
    if (!out) return fail(fn, "out is required");
    if (int rc = check_shape(fn, plan, y, WIDE_MAXE)) return rc;
    if (plan->num_nodes <= MAXE) {
        out[0] = y.W_fwd; out[1] = (int64_t)y.lds_fwd; out[2] = y.nblocks_fwd;
        return GMPE_OK;
    }
    WideLayout w;
    if (int rc = wide_layout(fn, plan, y, w)) return rc;
    out[0] = w.W; out[1] = (int64_t)w.lds; out[2] = w.nblocks;
    return GMPE_OK;
}

int gmpe_gnn_forward_wide(int device, const gmpe_gnn_plan* pl, void* stream) {
    const char* fn = "gmpe_gnn_forward_wide";
    Layout y = {};
    if (int rc = check_plan(fn, pl, false, y, false, WIDE_MAXE)) return rc;
    if (pl->num_nodes <= MAXE) return gmpe_gnn_forward(device, pl, stream);
    WideLayout w;
    if (int rc = wide_layout(fn, pl, y, w)) return rc;
    return launch_wide(device, w, bind(pl, y, false), 0, stream);
}

int gmpe_gnn_forward_wide_table(int device, const gmpe_gnn_table_plan* tp, void* stream) {
    const char* fn = "gmpe_gnn_forward_wide_table";
    Layout y = {};
    gmpe_gnn_plan base;
    if (int rc = check_table_plan(fn, tp, false, y, base, WIDE_MAXE)) return rc;
    if (base.num_nodes <= MAXE) return gmpe_gnn_forward_table(device, tp, stream);
    WideLayout w;
    if (int rc = wide_layout(fn, &base, y, w)) return rc;
    return launch_wide(device, w, bind_table(tp, base, y, false), 1, stream);
}

}  // extern "C"
