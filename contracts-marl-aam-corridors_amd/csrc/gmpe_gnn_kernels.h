// gmpe_gnn_kernels.h — the geometry, the kernels and the host half of the three files that run the policy's GNNBase: gmpe_gnn.hip (a graph's inputs are
// node rows and an adjacency: the GnnArgs instantiations), gmpe_gnn_table.hip (they are built from an entity table: the GnnTableArgs ones) and
// gmpe_gnn_wide.hip (the forward of both sources on graphs of 65 .. 128 nodes). Each of them includes this file alone and adds its kernel instantiations
// and its extern "C" entries. Everything here has internal linkage.
// The two sources are two translation units because both backward kernels use all 512 registers of a lane: with both sources in one kernel, or with the
// table's fields as ordinary arguments next to the rows', they spill (DESIGN.md 3.13 has the counts).
//
// The policy's GNNBase, forward and backward (include/gmpe.h gmpe_gnn_forward / gmpe_gnn_backward and their _table forms): GNNBase.forward
// (onpolicy/algorithms/utils/gnn_new.py:492-510) of one module — process_adj, the EmbedConv with its per-edge MLP, 1 + gnn_layer_N TransformerConv layers,
// the gather or the pool — as ONE forward launch and THREE backward launches, whatever rows, E and the data. No edge list is built: the dense matrix is the
// mask and the edge attribute.
//
// Mapping. A workgroup has four waves and owns tiles of W graphs (W = 1 .. 4: as many graphs' state as fits the LDS next to the weights, layout()), tile
// blockIdx.x, blockIdx.x + gridDim.x, ...; wave w < W owns graph w of the tile and lane i owns node i of it: its 16 channels are registers, and a lane's
// loop over the nodes j = 0 .. E-1 is the loop over its incoming (forward) or outgoing (backward) edges, the masked matrix standing in the wave's LDS at an
// odd row stride so that both directions read conflict-free. All parameters stand in LDS for the workgroup's lifetime, in the order of the header's
// workspace row (35 KiB at the shipped sizes); a lane reads them at wave-uniform addresses, as 16-byte broadcasts. What other lanes need of a node (its
// part P_j of lin1, its key and value of the current head, in backward its query, the head's output gradient and the softmax statistics) is in the wave's
// LDS, one head at a time. Every loop bound is the same in every wave, so the workgroup barriers are uniform; a wave without a graph computes nothing.
//
// The arithmetic of one graph is written in include/gmpe.h; it is a function of E and the configuration alone. What cancels is formed in double from float32
// values and rounded once (the LayerNorm's statistics, a node's sums over its edges, backward's softmax and dot products): DESIGN.md 3.13 has what each cost. Backward recomputes a graph's forward (the
// same code, the same bits), keeps each conv's input in LDS and walks back: the pool, each conv (softmax backward per target node in the target's lane, the
// key / value / edge gradients in the source's lane, the logits recomputed), then, in a launch of its own (the two halves' register sets do not fit one kernel without scratch), the per-edge MLP recomputed in registers in the
// source's lane, from the gradient of the EmbedConv's output that the first launch left in the workspace.
//
// Parameter gradients (no atomics). Every element belongs to one thread of the workgroup: element t of each 16 x 16 block (a weight matrix, a head's slice
// of one, 16 columns of lin1, the embedding table) and entry t % 16 of the 16-wide vectors g with g % 16 == t / 16. The operands are staged in LDS as rows
// [node][16]; the owner adds their exact double products over the tile's graphs in wave order and a graph's rows in ascending order, from 0, then adds that
// to its running double sum (a float32 chain over a graph's nodes cost the bias-like gradients 4 x the float32 reference's error at 300 graphs of 20 nodes:
// the partial sums grow, every add rounds to their size). The per-edge layers stage once per target node, everything else once per graph (its per-edge
// terms summed in the source's lane first, targets ascending, in double, and rounded once when staged). k_gnn_finish adds the workgroups in ascending order and rounds to float32 once.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "gmpe_expand.h"        // a node row and an adjacency entry from an entity table, with the engine's bits
#include "gmpe_host.h"          // include/gmpe.h, the error text, GMPE_HIP_CHECK, the layer files' shared host half

#pragma clang fp contract(off)

namespace {

// the geometry (tests/gnn_lib.py restates it from here)
constexpr int C = GMPE_GNN_HIDDEN, BLOCK = 256, NW = BLOCK / 64;
constexpr int MAXE = GMPE_GNN_MAX_NODES, MAXH = GMPE_GNN_MAX_HEADS, MAXC = GMPE_GNN_MAX_CONVS, MAXL = GMPE_GNN_MAX_EMBED_LAYERS;
constexpr int NINS = 32;                                // row stride of a node's lin1 input in LDS: F - 1 + embedding_size <= 23 columns, zeros behind
constexpr int QDS = 40;                                 // backward's per-node row: q [16], the head's output gradient [16], max, -, 1 / sum and D (doubles), -
constexpr int LIN = C * C + C;                          // a 16 x 16 Linear with its bias
// the wide forward (gmpe_gnn_wide.hip): a node per thread of a pair of waves, a graph per pair
constexpr int WIDE_MAXE = GMPE_GNN_WIDE_MAX_NODES, PAIR = 2 * 64, NPAIR = BLOCK / PAIR;
using gmpe::LDS_CU;
static_assert(C == 16 && NW == 4 && MAXH == 4 && MAXC == 3 && MAXL == 2, "16 channels, four waves");
static_assert(WIDE_MAXE == PAIR && NPAIR == 2, "a node per thread of a wave pair, two pairs in a workgroup");
static_assert(GMPE_GNN_MAX_FEATS - 1 + GMPE_GNN_MAX_EMBEDDING_SIZE <= NINS, "a node's lin1 input fits its LDS row");

// 16 x 16 blocks of parameter gradients (one element per thread) and 16-wide vectors (thread t owns entry t % 16 of the groups g with g % 16 == t / 16)
constexpr int B_EMB = 0, B_W1A = 1, B_W1B = 2, B_WL = 3, B_CONV = 5, B_PER_CONV = 3 * MAXH + 1;
constexpr int G_B1 = 0, G_W1E = 1, G_LNW = 2, G_LNB = 3, G_BL = 4, G_CONV = 6, G_PER_CONV = 4 * MAXH + 1;

// the parameters as one row of floats: the LDS image, and a workgroup's row of double sums in the workspace
struct Lay { int emb, w1, b1, lnw, lnb, wl, conv, cs, np; };
__host__ __device__ inline Lay lay_of(int nemb, int esz, int K1, int H, int nconv, int nel) {
    Lay L;
    L.emb = 0; L.w1 = (nemb * esz + 3) & ~3; L.b1 = L.w1 + C * K1; L.lnw = L.b1 + C; L.lnb = L.lnw + C; L.wl = L.lnb + C;
    L.conv = L.wl + nel * LIN; L.cs = 3 * H * LIN + H * C + LIN; L.np = L.conv + nconv * L.cs;
    return L;
}
// inside a conv's slice: m = 0 query, 1 key, 2 value
__host__ __device__ inline int cw(int H, int m, int h) { return m * H * LIN + h * C * C; }
__host__ __device__ inline int cb(int H, int m, int h) { return m * H * LIN + H * C * C + h * C; }
__host__ __device__ inline int cwe(int H, int h) { return 3 * H * LIN + h * C; }
__host__ __device__ inline int cws(int H) { return 3 * H * LIN + H * C; }
__host__ __device__ inline int cbs(int H) { return 3 * H * LIN + H * C + C * C; }

// a wave's own LDS, in floats
struct WLay { int ev, nin, P, xs, kv, qd, st, total; };
__host__ __device__ inline WLay wlay_of(int E, int nconv, bool bwd) {
    WLay w;
    const auto r4 = [](int v) { return (v + 3) & ~3; };
    w.ev = 0; w.nin = r4(E * (E | 1)); w.P = w.nin + E * NINS; w.xs = w.P + E * C; w.kv = w.xs + (bwd ? nconv + 1 : 1) * E * C;
    w.qd = w.kv + E * 2 * C; w.st = w.qd + (bwd ? E * QDS : 0); w.total = w.st + (bwd ? 4 * E * C : 0);
    return w;
}

struct ConvPtr { const float *wq, *bq, *wk, *bk, *wv, *bv, *we, *ws, *bs; float *gwq, *gbq, *gwk, *gbk, *gwv, *gbv, *gwe, *gws, *gbs; };
struct GnnArgs {
    int64_t rows, ntiles;
    int E, F, S, H, nconv, nel, eact, cact, ln, aggr, nemb, esz, K1, W, nblocks;
    float maxd, lneps;
    const float *x, *adj;
    const int32_t* id;
    const float *emb, *w1, *b1, *lnw, *lnb, *wl[MAXL], *bl[MAXL];
    float *gemb, *gw1, *gb1, *glnw, *glnb, *gwl[MAXL], *gbl[MAXL];
    ConvPtr cv[MAXC];
    float* out;
    const float* gout;
    double* part;                                       // workspace: [nblocks][np]
    float* dX;                                          // ... and the gradient of the EmbedConv's output [rows][E][16]
};

// The arguments of gmpe_gnn_table.hip's kernels. The table source stands in place of x and adj: graph g is the view of ego id[g] of table row tidx[g], or
// g / tshare without an index.
struct GnnTableArgs : GnnArgs {
    const double* tab;                                  // [tlast + 1][TW]
    const void* tidx;                                   // [rows] int32 or int64 (idx64), or null
    int64_t tlast;                                      // table_rows - 1
    int idx64, tshare, kind, two, A, NL, TW;            // gmpe_expand.h's KIND, two, A, L and W
};

// Tanh: the double function rounded once (tanhf is good to an ulp or two, and the derivative 1 - y^2 of a saturated unit multiplies y's error by 2 y / (1 - y^2));
// the derivative as (1 - y)(1 + y), whose first factor is exact for y >= 1/2, not 1 - y * y, whose product rounds at the size of 1.
__device__ __forceinline__ float activate(int act, float a) { return act == GMPE_GNN_RELU ? (a > 0.0f ? a : 0.0f) : (float)tanh((double)a); }
__device__ __forceinline__ float act_grad(int act, float y, float g) { return act == GMPE_GNN_RELU ? (y > 0.0f ? g : 0.0f) : g * ((1.0f - y) * (1.0f + y)); }

// The parameters in LDS are loop-invariant loads, and hoisted out of an edge loop they would pin hundreds of registers: nothing read from memory before this
// point is reused after it (no instruction is emitted).
__device__ __forceinline__ void reload() { __asm__ volatile("" ::: "memory"); }
// ... and a chain's result is formed here, not sunk into a later branch with its sixteen weights kept alive for it
__device__ __forceinline__ void pin(float& v) { __asm__ volatile("" : "+v"(v)); }
__device__ __forceinline__ void pin(double& v) { __asm__ volatile("" : "+v"(v)); }

__device__ __forceinline__ void load16(const float* s, float (&v)[C]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 t = *reinterpret_cast<const float4*>(s + 4 * q);
        v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
    }
}
__device__ __forceinline__ void store16(float* d, const float (&v)[C]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) *reinterpret_cast<float4*>(d + 4 * q) = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
}
template <class T>
__device__ __forceinline__ void zero16(T (&v)[C]) {
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = (T)0;
}
// a lane's double sums over its edges, rounded to float32 once, as a staged row
__device__ __forceinline__ void store16(float* d, const double (&v)[C]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) *reinterpret_cast<float4*>(d + 4 * q) = make_float4((float)v[4 * q], (float)v[4 * q + 1], (float)v[4 * q + 2], (float)v[4 * q + 3]);
}
// exact products, added in double, c ascending: backward's dot products, whose results are subtracted from one another
__device__ __forceinline__ double dot16(const float (&a)[C], const float (&b)[C]) {
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) s = fma((double)a[c], (double)b[c], s);
    return s;
}

// y[o] = fmaf chain from b[o] over k ascending of Wm[o][k] * x[k]
__device__ __forceinline__ void lin16(const float* Wm, const float* b, const float (&x)[C], float (&y)[C]) {
#pragma unroll
    for (int o = 0; o < C; ++o) {
        float w[C];
        load16(Wm + o * C, w);
        float a = b[o];
#pragma unroll
        for (int k = 0; k < C; ++k) a = fmaf(w[k], x[k], a);
        pin(a);
        y[o] = a;
        if ((o & 3) == 3) reload();
    }
}
// y[k] <- fmaf chain from y[k] over o ascending of Wm[o][k] * g[o]: the product with the transpose. T = double where several such products meet in one
// sum (a conv's input gradient: skip, and query, key and value of every head — up to 208 terms that cancel)
template <class T>
__device__ __forceinline__ void lin16T(const float* Wm, const float (&g)[C], T (&y)[C]) {
#pragma unroll
    for (int o = 0; o < C; ++o) {
        float w[C];
        load16(Wm + o * C, w);
#pragma unroll
        for (int k = 0; k < C; ++k) y[k] = (T)fma((T)w[k], (T)g[o], y[k]);
        if ((o & 3) == 3) {
#pragma unroll
            for (int k = 0; k < C; ++k) pin(y[k]);
            reload();
        }
    }
}

// what backward keeps of one edge's MLP: per stage (lin1, then the hidden layers) the activation, the normalised value and rstd
struct EdgeKept { float a[MAXL + 1][C], xh[MAXL + 1][C], rs[MAXL + 1]; };

// activation and the one LayerNorm over a lane's 16 values -> y
template <bool KEEP>
__device__ __forceinline__ void act_norm(const GnnArgs& p, const Lay& L, const float* Wt, const float (&pre)[C], float (&y)[C], EdgeKept* kp, int s) {
    float a[C];
#pragma unroll
    for (int c = 0; c < C; ++c) a[c] = activate(p.eact, pre[c]);
    if (KEEP) {
#pragma unroll
        for (int c = 0; c < C; ++c) kp->a[s][c] = a[c];
    }
    if (!p.ln) {
#pragma unroll
        for (int c = 0; c < C; ++c) y[c] = a[c];
        return;
    }
    // the statistics in double, the normalised value rounded once (as gmpe_mlp.hip's feature norm): a - mean loses the digits a float32 mean lacks
    double sum = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) sum += (double)a[c];
    const double mean = sum * (1.0 / C);
    double q = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) { const double d = (double)a[c] - mean; q = fma(d, d, q); }
    const double rstd = 1.0 / sqrt(q * (1.0 / C) + (double)p.lneps);
    float lw[C], lb[C];
    load16(Wt + L.lnw, lw); load16(Wt + L.lnb, lb);
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float xh = (float)(((double)a[c] - mean) * rstd);
        if (KEEP) kp->xh[s][c] = xh;
        y[c] = xh * lw[c] + lb[c];
    }
    if (KEEP) kp->rs[s] = (float)rstd;
}

// one edge's MLP: P = the source node's part of lin1, e the edge attribute, w1e lin1's last column
template <bool KEEP>
__device__ __forceinline__ void edge_forward(const GnnArgs& p, const Lay& L, const float* Wt, const float (&P)[C], const float (&w1e)[C], float e,
                                             float (&y)[C], EdgeKept* kp) {
    float pre[C];
#pragma unroll
    for (int c = 0; c < C; ++c) pre[c] = fmaf(w1e[c], e, P[c]);
    act_norm<KEEP>(p, L, Wt, pre, y, kp, 0);
#pragma unroll
    for (int l = 0; l < MAXL; ++l)
        if (l < p.nel) {
            lin16(Wt + L.wl + l * LIN, Wt + L.wl + l * LIN + C * C, y, pre);
            act_norm<KEEP>(p, L, Wt, pre, y, kp, l + 1);
        }
}

// stage s of an edge's MLP backward: g, the gradient of the stage's output -> the gradient of its pre-activation; the LayerNorm's sums into the lane's
__device__ __forceinline__ void act_norm_backward(const GnnArgs& p, const Lay& L, const float* Wt, const EdgeKept& kp, int s, const float (&g)[C],
                                                  float (&dpre)[C], double (&dlnw)[C], double (&dlnb)[C]) {
    float da[C];
    if (p.ln) {                                         // the two means and the difference that cancels against them in double, rounded once
        float lw[C];
        load16(Wt + L.lnw, lw);
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            dlnw[c] = fma((double)g[c], (double)kp.xh[s][c], dlnw[c]);
            dlnb[c] += (double)g[c];
            const double dxh = (double)g[c] * (double)lw[c];
            s1 += dxh;
            s2 = fma(dxh, (double)kp.xh[s][c], s2);
        }
        s1 *= 1.0 / C; s2 *= 1.0 / C;
#pragma unroll
        for (int c = 0; c < C; ++c)
            da[c] = (float)((double)kp.rs[s] * (((double)g[c] * (double)lw[c] - s1) - (double)kp.xh[s][c] * s2));
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) da[c] = g[c];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) dpre[c] = act_grad(p.eact, kp.a[s][c], da[c]);
}

// the output of stage s again, with forward's roundings
__device__ __forceinline__ void stage_output(const GnnArgs& p, const Lay& L, const float* Wt, const EdgeKept& kp, int s, float (&y)[C]) {
    if (p.ln) {
        float lw[C], lb[C];
        load16(Wt + L.lnw, lw); load16(Wt + L.lnb, lb);
#pragma unroll
        for (int c = 0; c < C; ++c) y[c] = kp.xh[s][c] * lw[c] + lb[c];
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) y[c] = kp.a[s][c];
    }
}

// the logit of edge j -> i and the edge's value vector: kc = k_j + ee, vc = v_j + ee
__device__ __forceinline__ float edge_logit(const float (&q)[C], const float (&k)[C], const float (&we)[C], float e) {
    float s = 0.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) s = fmaf(q[c], fmaf(we[c], e, k[c]), s);
    return s * 0.25f;
}

// the parameters into LDS in Lay's order
__device__ __forceinline__ void load_params(const GnnArgs& p, const Lay& L, float* Wt, int tid) {
    const auto copy = [&](const float* src, int off, int n) {
#pragma unroll 1
        for (int i = tid; i < n; i += BLOCK) Wt[off + i] = src[i];
    };
    copy(p.emb, L.emb, p.nemb * p.esz);
    copy(p.w1, L.w1, C * p.K1);
    copy(p.b1, L.b1, C);
    if (p.ln) { copy(p.lnw, L.lnw, C); copy(p.lnb, L.lnb, C); }
#pragma unroll
    for (int l = 0; l < MAXL; ++l)
        if (l < p.nel) { copy(p.wl[l], L.wl + l * LIN, C * C); copy(p.bl[l], L.wl + l * LIN + C * C, C); }
    const int H = p.H;
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
        if (c < p.nconv) {
            const int o = L.conv + c * L.cs;
            const ConvPtr& v = p.cv[c];
            copy(v.wq, o + cw(H, 0, 0), H * C * C); copy(v.bq, o + cb(H, 0, 0), H * C);
            copy(v.wk, o + cw(H, 1, 0), H * C * C); copy(v.bk, o + cb(H, 1, 0), H * C);
            copy(v.wv, o + cw(H, 2, 0), H * C * C); copy(v.bv, o + cb(H, 2, 0), H * C);
            copy(v.we, o + cwe(H, 0), H * C); copy(v.ws, o + cws(H), C * C); copy(v.bs, o + cbs(H), C);
        }
}

// The node mapping of the functions below: thread s of the ns that stage a graph's matrix; `node`, the node this thread owns, and `owner`, whether it
// computes a node at all. A narrow kernel passes lane, 64, lane, true (a graph per wave); k_gnn_fwd_wide its thread of a pair of waves. `on`, this thread
// owns a node of a graph, is formed from them in each function: handed down as a finished predicate it costs k_gnn_bwd_embed its last registers
// (DESIGN.md 3.13a).
//
// What a graph's source gives: the masked matrix into ev (all staging threads of an active graph) and, with `on`, the first F - 1 features of this thread's
// node into its lin1 input row nin -> its type as the float the rows hold. From the rows and the adjacency:
__device__ __forceinline__ float graph_source(const GnnArgs& p, float* ev, float* nin, int s, int ns, int node, int64_t g, bool on) {
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
// ... and from an entity table, with gmpe_expand.h's arithmetic (the engine's bits): entry (j, i) of the env-step's matrix, and the row of entity `node` as
// ego id[g] sees it. The helpers write a whole row, the type last, into nin (16-byte aligned, as KIND 0's float4 stores need); the caller overwrites the
// type's place with the embedding, as it does behind the copied rows.
__device__ __forceinline__ float graph_source(const GnnTableArgs& p, float* ev, float* nin, int s, int ns, int node, int64_t g, bool on) {
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

// A graph's inputs into its LDS block wl: the masked matrix, every node's lin1 input row and its part P of lin1. Every wave of the workgroup calls it
// together (it ends in a workgroup barrier). -> P, this thread's node's part; type, its clamped entity type. ARGS: GnnArgs or GnnTableArgs, the source.
template <class ARGS>
__device__ __forceinline__ void graph_inputs(const ARGS& p, const Lay& L, const WLay& WL, const float* Wt, float* wl, int s, int ns, int node, bool owner,
                                             int64_t g, bool active, float (&P)[C], int& type) {
    const int E = p.E;
    const bool on = active && owner && node < E;
    float* nin = wl + WL.nin + node * NINS;
    float tf = 0.0f;
    if (active) tf = graph_source(p, wl + WL.ev, nin, s, ns, node, g, on);
    type = 0;
    if (on) {
        type = tf >= 1.0f ? (tf < (float)p.nemb ? (int)tf : p.nemb - 1) : 0;           // int() truncates; NaN and everything outside go to the ends
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

// One graph's forward for the threads of its block wl; every wave of the workgroup calls it together (it holds workgroup barriers).
// -> x, the node's row of the last layer (also in the block's xs[KEEP ? nconv : 0]).
template <bool KEEP, class ARGS>
__device__ __forceinline__ void graph_forward(const ARGS& p, const Lay& L, const WLay& WL, const float* Wt, float* wl, int s, int ns, int node, bool owner,
                                              int64_t g, bool active, float (&x)[C]) {
    const int E = p.E, es = E | 1, H = p.H;
    const bool on = active && owner && node < E;
    const float* ev = wl + WL.ev;
    {
        float P[C];
        int type;
        graph_inputs(p, L, WL, Wt, wl, s, ns, node, owner, g, active, P, type);
    }
    double xa[C];                                       // a node's sum over its incoming edges in double, rounded once
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
    const float Hf = (float)H;
    for (int cc = 0; cc < p.nconv; ++cc) {
        const float* Wc = Wt + L.conv + cc * L.cs;
        float sk[C], o[C];
        zero16(o);
        if (on) {
            if (KEEP) store16(wl + WL.xs + (cc * E + node) * C, x);
            lin16(Wc + cws(H), Wc + cbs(H), x, sk);
        }
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
            __syncthreads();                            // the next head's keys and values take this head's place
        }
        if (on) {
#pragma unroll
            for (int c = 0; c < C; ++c) x[c] = activate(p.cact, __fdiv_rn(o[c], Hf) + sk[c]);
        }
    }
    if (on) store16(wl + WL.xs + ((KEEP ? p.nconv : 0) * E + node) * C, x);
    __syncthreads();
}

__device__ __forceinline__ int ego_of(const GnnArgs& p, int64_t g) {
    const int id = p.id[g];
    return id < 0 ? 0 : (id >= p.E ? p.E - 1 : id);
}

// the gather or the pool of graph g over the rows xs that graph_forward<false> left: one thread per channel, the nodes ascending
__device__ __forceinline__ void graph_output(const GnnArgs& p, const float* xs, int channel, int64_t g) {
    float r;
    if (p.aggr == GMPE_GNN_NODE) r = xs[ego_of(p, g) * C + channel];
    else {
        r = xs[channel];
#pragma unroll 1
        for (int i = 1; i < p.E; ++i) {
            reload();
            const float v = xs[i * C + channel];
            r = p.aggr == GMPE_GNN_MAX ? (v > r ? v : r) : r + v;
        }
        if (p.aggr == GMPE_GNN_MEAN) r = __fdiv_rn(r, (float)p.E);
    }
    p.out[g * C + channel] = r;
}

template <class ARGS>
__global__ __launch_bounds__(BLOCK) void k_gnn_fwd(ARGS p) {
    extern __shared__ __attribute__((aligned(16))) float sh[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const Lay L = lay_of(p.nemb, p.esz, p.K1, p.H, p.nconv, p.nel);
    const WLay WL = wlay_of(p.E, p.nconv, false);
    float* wl = sh + L.np + wv * WL.total;
    load_params(p, L, sh, tid);
    __syncthreads();
    for (int64_t tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
        const int64_t g = tile * p.W + wv;
        const bool active = wv < p.W && g < p.rows;
        float x[C];
        graph_forward<false>(p, L, WL, sh, wl, lane, 64, lane, true, g, active, x);
        if (active && lane < C) graph_output(p, wl + WL.xs, lane, g);
        __syncthreads();                                // the next tile overwrites the waves' state
    }
}

// the owner's share of a staged product: exact double products, the tile's graphs in wave order and a graph's nodes ascending
__device__ __forceinline__ double outer_sum(const float* w0, int wstride, int nw, int E, int aoff, int boff, int bstride, int r, int c) {
    double d = 0.0;
    for (int w = 0; w < nw; ++w) {
        const float* A = w0 + w * wstride + aoff;
        const float* B = w0 + w * wstride + boff;
#pragma unroll 1
        for (int e = 0; e < E; ++e) d = fma((double)A[e * C + r], (double)B[e * bstride + c], d);
    }
    return d;
}
__device__ __forceinline__ double column_sum(const float* w0, int wstride, int nw, int E, int aoff, int c) {
    double d = 0.0;
    for (int w = 0; w < nw; ++w) {
        const float* A = w0 + w * wstride + aoff;
#pragma unroll 1
        for (int e = 0; e < E; ++e) d += (double)A[e * C + c];
    }
    return d;
}
// acc[b] += d with the index resolved into registers: a uniform compare per element
template <int N>
__device__ __forceinline__ void add_at(double (&acc)[N], int b, double d) {
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] += k == b ? d : 0.0;
}

constexpr int NBC = MAXC * B_PER_CONV, NVC = (MAXC * G_PER_CONV + 15) / 16;           // the convs' blocks and vector groups, counted from B_CONV and G_CONV
static_assert(G_CONV <= 16, "the EmbedConv's vector groups are one entry per thread");

// backward 1 (the head of this file): a graph's forward again, the pool and the convs backward -> the gradient of the EmbedConv's output, dX
template <class ARGS>
__global__ __launch_bounds__(BLOCK) void k_gnn_bwd_conv(ARGS p) {
    extern __shared__ __attribute__((aligned(16))) float sh[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, E = p.E, es = E | 1, H = p.H;
    const int orow = tid >> 4, ocol = tid & 15;
    const Lay L = lay_of(p.nemb, p.esz, p.K1, H, p.nconv, p.nel);
    const WLay WL = wlay_of(E, p.nconv, true);
    float* w0 = sh + L.np;
    float* wl = w0 + wv * WL.total;
    const float* Wt = sh;
    load_params(p, L, sh, tid);
    __syncthreads();
    double blk[NBC], vec[NVC];                          // this thread's share of the convs' parameter gradients
#pragma unroll
    for (int k = 0; k < NBC; ++k) blk[k] = 0.0;
#pragma unroll
    for (int k = 0; k < NVC; ++k) vec[k] = 0.0;
    const auto block_add = [&](int b, int aoff, int boff, int bstride, int nw) {
        add_at(blk, b - B_CONV, outer_sum(w0, WL.total, nw, E, aoff, boff, bstride, orow, ocol));
    };
    const auto group_add = [&](int g, int aoff, int nw) {
        if (((g - G_CONV) & 15) == orow) add_at(vec, (g - G_CONV) >> 4, column_sum(w0, WL.total, nw, E, aoff, ocol));
    };
    const float Hf = (float)H;
    for (int64_t tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
        const int64_t g0 = tile * p.W, g = g0 + wv;
        const int64_t left = p.rows - g0;
        const int nw = left < p.W ? (int)left : p.W;    // the graphs of this tile
        const bool active = wv < nw, on = active && lane < E;
        float x[C], dy[C];
        graph_forward<true>(p, L, WL, Wt, wl, lane, 64, lane, true, g, active, x);
        const float* ev = wl + WL.ev;
        float* st = wl + WL.st;
        float* qd = wl + WL.qd;
        zero16(dy);
        if (on) {                                       // the gather's or the pool's backward
            float go[C];
            load16(p.gout + g * C, go);
            if (p.aggr == GMPE_GNN_NODE) {
                const bool me = ego_of(p, g) == lane;
#pragma unroll
                for (int c = 0; c < C; ++c) dy[c] = me ? go[c] : 0.0f;
            } else if (p.aggr == GMPE_GNN_MAX) {        // the first node that holds the maximum, as forward's scan keeps it
                const float* xs = wl + WL.xs + p.nconv * E * C;
                float m[C];
                int win[C];
                load16(xs, m);
#pragma unroll
                for (int c = 0; c < C; ++c) win[c] = 0;
#pragma unroll 1
                for (int i = 1; i < E; ++i) {
                    reload();
                    float v[C];
                    load16(xs + i * C, v);
#pragma unroll
                    for (int c = 0; c < C; ++c)
                        if (v[c] > m[c]) { m[c] = v[c]; win[c] = i; }
                }
#pragma unroll
                for (int c = 0; c < C; ++c) dy[c] = win[c] == lane ? go[c] : 0.0f;
            } else {
#pragma unroll
                for (int c = 0; c < C; ++c) dy[c] = p.aggr == GMPE_GNN_MEAN ? __fdiv_rn(go[c], (float)E) : go[c];
            }
        }
        for (int cc = p.nconv - 1; cc >= 0; --cc) {
            const float* Wc = Wt + L.conv + cc * L.cs;
            const int xin_off = WL.xs + cc * E * C;
            float xin[C], dz[C], dout[C];
            double dx[C];                               // exact products, one double sum over the skip and every head's three Linears, rounded once
            zero16(dx);
            if (on) {
                float y[C];
                load16(wl + xin_off + lane * C, xin);
                load16(wl + xin_off + (E + lane) * C, y);
#pragma unroll
                for (int c = 0; c < C; ++c) { dz[c] = act_grad(p.cact, y[c], dy[c]); dout[c] = __fdiv_rn(dz[c], Hf); }
                lin16T(Wc + cws(H), dz, dx);
                store16(st + lane * C, dz);
            }
            __syncthreads();
            block_add(B_CONV + cc * B_PER_CONV + 3 * MAXH, WL.st, xin_off, C, nw);
            group_add(G_CONV + cc * G_PER_CONV + 4 * MAXH, WL.st, nw);
            __syncthreads();
            for (int h = 0; h < H; ++h) {
                float q[C], k[C], v[C], we[C];
                if (on) {
                    lin16(Wc + cw(H, 0, h), Wc + cb(H, 0, h), xin, q);
                    lin16(Wc + cw(H, 1, h), Wc + cb(H, 1, h), xin, k);
                    lin16(Wc + cw(H, 2, h), Wc + cb(H, 2, h), xin, v);
                    load16(Wc + cwe(H, h), we);
                    store16(wl + WL.kv + lane * 2 * C, k);
                    store16(wl + WL.kv + lane * 2 * C + C, v);
                    store16(qd + lane * QDS, q);
                    store16(qd + lane * QDS + C, dout);
                }
                __syncthreads();
                double dq[C], dk[C], dv[C], dwe[C];     // sums over a node's edges, in double: rounded once when staged and when they enter dx
                zero16(dq); zero16(dk); zero16(dv); zero16(dwe);
                if (on) {                               // the target's lane: the softmax statistics, D = sum_j alpha_ji (dout_i . vc_ji), then dq
                    float m = -INFINITY;
#pragma unroll 1
                    for (int j = 0; j < E; ++j) {
                        reload();
                        const float e = ev[j * es + lane];
                        if (e > 0.0f) {
                            float kj[C];
                            load16(wl + WL.kv + j * 2 * C, kj);
                            const float l = edge_logit(q, kj, we, e);
                            m = l > m ? l : m;
                        }
                    }
                    // backward's own softmax: the sum in double and alpha = p / sum in double, so that sum_j alpha_ji (da_ji - D) is zero to double
                    // precision — in float32 what is left of it is multiplied by what the keys have in common
                    double sum = 0.0, U = 0.0;
#pragma unroll 1
                    for (int j = 0; j < E; ++j) {
                        reload();
                        const float e = ev[j * es + lane];
                        if (e > 0.0f) {
                            float kj[C], vj[C], vc[C];
                            load16(wl + WL.kv + j * 2 * C, kj);
                            load16(wl + WL.kv + j * 2 * C + C, vj);
                            const float pr = expf(edge_logit(q, kj, we, e) - m);
                            sum += (double)pr;
#pragma unroll
                            for (int c = 0; c < C; ++c) vc[c] = fmaf(we[c], e, vj[c]);
                            U = fma((double)pr, dot16(dout, vc), U);
                        }
                    }
                    const double rsum = sum > 0.0 ? 1.0 / sum : 0.0, D = U * rsum;
#pragma unroll 1
                    for (int j = 0; j < E; ++j) {
                        reload();
                        const float e = ev[j * es + lane];
                        if (e > 0.0f) {
                            float kj[C], vj[C], vc[C];
                            load16(wl + WL.kv + j * 2 * C, kj);
                            load16(wl + WL.kv + j * 2 * C + C, vj);
                            const double al = (double)expf(edge_logit(q, kj, we, e) - m) * rsum;
#pragma unroll
                            for (int c = 0; c < C; ++c) vc[c] = fmaf(we[c], e, vj[c]);
                            const double t = (al * (dot16(dout, vc) - D)) * 0.25;
#pragma unroll
                            for (int c = 0; c < C; ++c) dq[c] = fma(t, (double)fmaf(we[c], e, kj[c]), dq[c]);
                        }
                    }
                    qd[lane * QDS + 2 * C] = m;
                    *reinterpret_cast<double*>(qd + lane * QDS + 2 * C + 2) = rsum;
                    *reinterpret_cast<double*>(qd + lane * QDS + 2 * C + 4) = D;
                }
                __syncthreads();
                if (on) {                               // the source's lane: its key, value and edge terms over its targets ascending
#pragma unroll 1
                    for (int i = 0; i < E; ++i) {
                        reload();
                        const float e = ev[lane * es + i];
                        if (e > 0.0f) {
                            float qi[C], di[C], vc[C];
                            const float* row = qd + i * QDS;
                            load16(row, qi);
                            load16(row + C, di);
                            const float m = row[2 * C];
                            const double rsum = *reinterpret_cast<const double*>(row + 2 * C + 2), D = *reinterpret_cast<const double*>(row + 2 * C + 4);
                            const double al = (double)expf(edge_logit(qi, k, we, e) - m) * rsum;
#pragma unroll
                            for (int c = 0; c < C; ++c) vc[c] = fmaf(we[c], e, v[c]);
                            const double t = (al * (dot16(di, vc) - D)) * 0.25;
#pragma unroll
                            for (int c = 0; c < C; ++c) {
                                dk[c] = fma(t, (double)qi[c], dk[c]);
                                dv[c] = fma(al, (double)di[c], dv[c]);
                                dwe[c] = fma(t * (double)qi[c] + al * (double)di[c], (double)e, dwe[c]);
                            }
                        }
                    }
                    float r[C];
#pragma unroll
                    for (int c = 0; c < C; ++c) r[c] = (float)dq[c];
                    lin16T(Wc + cw(H, 0, h), r, dx);
#pragma unroll
                    for (int c = 0; c < C; ++c) r[c] = (float)dk[c];
                    lin16T(Wc + cw(H, 1, h), r, dx);
#pragma unroll
                    for (int c = 0; c < C; ++c) r[c] = (float)dv[c];
                    lin16T(Wc + cw(H, 2, h), r, dx);
                    store16(st + lane * C, dq);
                    store16(st + (E + lane) * C, dk);
                    store16(st + (2 * E + lane) * C, dv);
                    store16(st + (3 * E + lane) * C, dwe);
                }
                __syncthreads();
#pragma unroll
                for (int m = 0; m < 3; ++m) {
                    block_add(B_CONV + cc * B_PER_CONV + 3 * h + m, WL.st + m * E * C, xin_off, C, nw);
                    group_add(G_CONV + cc * G_PER_CONV + 4 * h + m, WL.st + m * E * C, nw);
                }
                group_add(G_CONV + cc * G_PER_CONV + 4 * h + 3, WL.st + 3 * E * C, nw);
                __syncthreads();
            }
#pragma unroll
            for (int c = 0; c < C; ++c) dy[c] = (float)dx[c];
        }
        if (on) store16(p.dX + (g * E + lane) * C, dy);
        __syncthreads();                                // the next tile overwrites the waves' state
    }
    double* row = p.part + (int64_t)blockIdx.x * L.np;
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
        if (c < p.nconv) {
            const int o = L.conv + c * L.cs;
#pragma unroll
            for (int h = 0; h < MAXH; ++h)
                if (h < H) {
#pragma unroll
                    for (int m = 0; m < 3; ++m) row[o + cw(H, m, h) + tid] = blk[c * B_PER_CONV + 3 * h + m];
                }
            row[o + cws(H) + tid] = blk[c * B_PER_CONV + 3 * MAXH];
        }
#pragma unroll
    for (int k = 0; k < NVC; ++k) {
        const int gi = 16 * k + orow;
        const int c = gi / G_PER_CONV, r = gi % G_PER_CONV, h = r >> 2, m = r & 3, o = L.conv + c * L.cs;
        int at = -1;
        if (c < p.nconv) {
            if (r == 4 * MAXH) at = o + cbs(H) + ocol;
            else if (h < H) at = m < 3 ? o + cb(H, m, h) + ocol : o + cwe(H, h) + ocol;
        }
        if (at >= 0) row[at] = vec[k];
    }
}

// backward 2: the EmbedConv. This lane is the source j of its edges, targets ascending: the edge's MLP again, then back through it.
template <class ARGS>
__global__ __launch_bounds__(BLOCK) void k_gnn_bwd_embed(ARGS p) {
    extern __shared__ __attribute__((aligned(16))) float sh[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, E = p.E, es = E | 1;
    const int orow = tid >> 4, ocol = tid & 15;
    const Lay L = lay_of(p.nemb, p.esz, p.K1, p.H, p.nconv, p.nel);
    const WLay WL = wlay_of(E, p.nconv, true);
    float* w0 = sh + L.np;
    float* wl = w0 + wv * WL.total;
    const float* Wt = sh;
    load_params(p, L, sh, tid);
    __syncthreads();
    double blk[B_CONV], vec = 0.0;                      // this thread's share of the EmbedConv's parameter gradients
#pragma unroll
    for (int k = 0; k < B_CONV; ++k) blk[k] = 0.0;
    const auto block_add = [&](int b, int aoff, int boff, int bstride, int nw) { add_at(blk, b, outer_sum(w0, WL.total, nw, E, aoff, boff, bstride, orow, ocol)); };
    const auto group_add = [&](int g, int aoff, int nw) {
        if (g == orow) vec += column_sum(w0, WL.total, nw, E, aoff, ocol);
    };
    for (int64_t tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
        const int64_t g0 = tile * p.W, g = g0 + wv;
        const int64_t left = p.rows - g0;
        const int nw = left < p.W ? (int)left : p.W;
        const bool active = wv < nw, on = active && lane < E;
        float P[C];
        int type;
        graph_inputs(p, L, WL, Wt, wl, lane, 64, lane, true, g, active, P, type);
        const float* ev = wl + WL.ev;
        float* st = wl + WL.st;
        float* qd = wl + WL.qd;
        if (on) {
            float dy[C];
            load16(p.dX + (g * E + lane) * C, dy);
            store16(qd + lane * C, dy);
        }
        __syncthreads();
        double dP[C], dw1e[C], dlnw[C], dlnb[C], dbl[MAXL][C];   // this source's sums over its edges, in double: rounded once when staged
        float w1e[C];
        zero16(dP); zero16(dw1e); zero16(dlnw); zero16(dlnb);
#pragma unroll
        for (int l = 0; l < MAXL; ++l) zero16(dbl[l]);
#pragma unroll
        for (int c = 0; c < C; ++c) w1e[c] = Wt[L.w1 + c * p.K1 + p.K1 - 1];
#pragma unroll 1
        for (int i = 0; i < E; ++i) {
            reload();
            const float e = on ? ev[lane * es + i] : 0.0f;
            if (e > 0.0f) {
                EdgeKept kp;
                float y[C], gr[C], dpre[C];
                edge_forward<true>(p, L, Wt, P, w1e, e, y, &kp);
                load16(qd + i * C, gr);
#pragma unroll
                for (int l = MAXL - 1; l >= 0; --l)
                    if (l < p.nel) {
                        act_norm_backward(p, L, Wt, kp, l + 1, gr, dpre, dlnw, dlnb);
                        stage_output(p, L, Wt, kp, l, y);
#pragma unroll
                        for (int c = 0; c < C; ++c) dbl[l][c] += (double)dpre[c];
                        store16(st + (2 * l * E + lane) * C, dpre);
                        store16(st + ((2 * l + 1) * E + lane) * C, y);
                        zero16(gr);
                        lin16T(Wt + L.wl + l * LIN, dpre, gr);
                    }
                act_norm_backward(p, L, Wt, kp, 0, gr, dpre, dlnw, dlnb);
#pragma unroll
                for (int c = 0; c < C; ++c) { dP[c] += (double)dpre[c]; dw1e[c] = fma((double)dpre[c], (double)e, dw1e[c]); }
            } else if (on) {
                float z[C];
                zero16(z);
                for (int l = 0; l < 2 * p.nel; ++l) store16(st + (l * E + lane) * C, z);
            }
            if (p.nel > 0) {
                __syncthreads();
#pragma unroll
                for (int l = 0; l < MAXL; ++l)
                    if (l < p.nel) block_add(B_WL + l, WL.st + 2 * l * E * C, WL.st + (2 * l + 1) * E * C, C, nw);
                __syncthreads();
            }
        }
        if (on) {
            store16(st + lane * C, dP);
            store16(st + (E + lane) * C, dw1e);
            store16(st + (2 * E + lane) * C, dlnw);
            store16(st + (3 * E + lane) * C, dlnb);
        }
        __syncthreads();
        block_add(B_W1A, WL.st, WL.nin, NINS, nw);
        block_add(B_W1B, WL.st, WL.nin + C, NINS, nw);
        group_add(G_B1, WL.st, nw);
        group_add(G_W1E, WL.st + E * C, nw);
        group_add(G_LNW, WL.st + 2 * E * C, nw);
        group_add(G_LNB, WL.st + 3 * E * C, nw);
        __syncthreads();
        if (on) {                                       // the embedding table: one-hot(type) x (lin1's embedding columns, transposed, times dP)
            float* hot = st + lane * C;
            float* de = st + (E + lane) * C;
#pragma unroll
            for (int c = 0; c < C; ++c) hot[c] = c == type ? 1.0f : 0.0f;
            for (int k = 0; k < C; ++k) {
                double s = 0.0;                         // in double from the double dP: the sum cancels, and a float32 dP's rounding would show
                if (k < p.esz) {
#pragma unroll
                    for (int c = 0; c < C; ++c) s = fma((double)Wt[L.w1 + c * p.K1 + p.F - 1 + k], dP[c], s);
                }
                de[k] = (float)s;
            }
            store16(st + (2 * E + lane) * C, dbl[0]);
            store16(st + (3 * E + lane) * C, dbl[1]);
        }
        __syncthreads();
        block_add(B_EMB, WL.st, WL.st + E * C, C, nw);
        group_add(G_BL, WL.st + 2 * E * C, nw);
        group_add(G_BL + 1, WL.st + 3 * E * C, nw);
        __syncthreads();                                // the next tile overwrites the waves' state
    }
    // the thread's sums into the workgroup's row, at the parameters' places
    double* row = p.part + (int64_t)blockIdx.x * L.np;
    if (orow < p.nemb && ocol < p.esz) row[L.emb + orow * p.esz + ocol] = blk[B_EMB];
    if (ocol < p.K1 - 1) row[L.w1 + orow * p.K1 + ocol] = blk[B_W1A];
    if (C + ocol < p.K1 - 1) row[L.w1 + orow * p.K1 + C + ocol] = blk[B_W1B];
#pragma unroll
    for (int l = 0; l < MAXL; ++l)
        if (l < p.nel) row[L.wl + l * LIN + tid] = blk[B_WL + l];
    int at = -1;
    if (orow == G_B1) at = L.b1 + ocol;
    else if (orow == G_W1E) at = L.w1 + ocol * p.K1 + p.K1 - 1;
    else if (orow == G_LNW) at = p.ln ? L.lnw + ocol : -1;
    else if (orow == G_LNB) at = p.ln ? L.lnb + ocol : -1;
    else if (orow < G_CONV) at = orow - G_BL < p.nel ? L.wl + (orow - G_BL) * LIN + C * C + ocol : -1;
    if (at >= 0) row[at] = vec;
}

// where element idx of Lay's row goes, or null (padding; the LayerNorm's places without LayerNorm)
__device__ __forceinline__ float* grad_place(const GnnArgs& p, const Lay& L, int idx) {
    const int H = p.H;
    if (idx < p.nemb * p.esz) return p.gemb + idx;
    if (idx < L.w1) return nullptr;
    if (idx < L.b1) return p.gw1 + (idx - L.w1);
    if (idx < L.lnw) return p.gb1 + (idx - L.b1);
    if (idx < L.lnb) return p.ln ? p.glnw + (idx - L.lnw) : nullptr;
    if (idx < L.wl) return p.ln ? p.glnb + (idx - L.lnb) : nullptr;
    if (idx < L.conv) {
        const int l = (idx - L.wl) / LIN, o = (idx - L.wl) % LIN;
        float* w = l == 0 ? p.gwl[0] : p.gwl[1];
        float* b = l == 0 ? p.gbl[0] : p.gbl[1];
        return o < C * C ? w + o : b + (o - C * C);
    }
    const int c = (idx - L.conv) / L.cs, o = (idx - L.conv) % L.cs;
    float* r = nullptr;
#pragma unroll
    for (int k = 0; k < MAXC; ++k)
        if (k == c) {
            const ConvPtr& v = p.cv[k];
            if (o < 3 * H * LIN) {
                const int m = o / (H * LIN), q = o % (H * LIN);
                float* w = m == 0 ? v.gwq : (m == 1 ? v.gwk : v.gwv);
                float* b = m == 0 ? v.gbq : (m == 1 ? v.gbk : v.gbv);
                r = q < H * C * C ? w + q : b + (q - H * C * C);
            } else if (o < cws(H)) r = v.gwe + (o - cwe(H, 0));
            else if (o < cbs(H)) r = v.gws + (o - cws(H));
            else r = v.gbs + (o - cbs(H));
        }
    return r;
}

// backward 3: the workgroups' sums in ascending order, rounded once
__global__ __launch_bounds__(BLOCK) void k_gnn_finish(GnnArgs p) {
    const Lay L = lay_of(p.nemb, p.esz, p.K1, p.H, p.nconv, p.nel);
    const int idx = blockIdx.x * BLOCK + threadIdx.x;
    if (idx >= L.np) return;
    float* dst = grad_place(p, L, idx);
    if (!dst) return;
    double s = 0.0;
#pragma unroll 1
    for (int b = 0; b < p.nblocks; ++b) s += p.part[(int64_t)b * L.np + idx];
    *dst = (float)s;
}

using gmpe::fail;

struct Layout {
    Lay L;
    int K1, W_fwd, W_bwd, nblocks_fwd, nblocks_bwd;
    int64_t ntiles_fwd, ntiles_bwd;
    size_t lds_fwd, lds_bwd, dX, total;
};

// the checks of the shape and the configuration, which the workspace size depends on. maxe: the nodes the calling entry is built for; above MAXE
// (gmpe_gnn_wide.hip's forward) the forward geometry is a graph per pair of waves and backward's fields stay zero: there is no backward.
int check_shape(const char* fn, const gmpe_gnn_plan* pl, Layout& y, int maxe = MAXE) {
    const auto range = [&](const char* name, int64_t v, int64_t lo, int64_t hi) {
        if (v < lo || v > hi)
            return fail(fn, std::string("unsupported ") + name + " = " + std::to_string(v) + ": " + std::to_string(lo) + " .. " + std::to_string(hi) + " are built");
        return (int)GMPE_OK;
    };
    if (!pl) return fail(fn, "null plan");
    if (pl->rows < 1 || pl->rows > (int64_t)1 << 40) return fail(fn, "rows must be >= 1 (and not absurd)");
    if (pl->hidden != C) return fail(fn, "unsupported hidden = " + std::to_string(pl->hidden) + ": only 16 is built");
    if (pl->concat != 0) return fail(fn, "unsupported concat = " + std::to_string(pl->concat) + ": only averaged heads are built");
    if (pl->beta != 0) return fail(fn, "unsupported beta = " + std::to_string(pl->beta) + ": only beta = 0 is built");
    if (pl->edge_dim != 1) return fail(fn, "unsupported edge_dim = " + std::to_string(pl->edge_dim) + ": only 1 is built");
    if (int rc = range("num_nodes", pl->num_nodes, 1, maxe)) return rc;
    if (int rc = range("node_feats", pl->node_feats, 2, GMPE_GNN_MAX_FEATS)) return rc;
    if (int rc = range("heads", pl->heads, 1, MAXH)) return rc;
    if (int rc = range("gnn_layer_n", pl->gnn_layer_n, 0, MAXC - 1)) return rc;
    if (int rc = range("embed_layer_n", pl->embed_layer_n, 0, MAXL)) return rc;
    if (int rc = range("num_embeddings", pl->num_embeddings, 1, GMPE_GNN_MAX_EMBEDDINGS)) return rc;
    if (int rc = range("embedding_size", pl->embedding_size, 1, GMPE_GNN_MAX_EMBEDDING_SIZE)) return rc;
    if (pl->adj_share < 1) return fail(fn, "adj_share must be >= 1");
    if (pl->rows % pl->adj_share) return fail(fn, "rows must be a multiple of adj_share");
    const int E = pl->num_nodes, nconv = pl->gnn_layer_n + 1;
    y = {};
    y.K1 = pl->node_feats - 1 + pl->embedding_size + 1;
    y.L = lay_of(pl->num_embeddings, pl->embedding_size, y.K1, pl->heads, nconv, pl->embed_layer_n);
    const bool wide = E > MAXE;
    const auto waves = [&](bool bwd, size_t& lds) {       // as many graphs side by side as the LDS holds next to the parameters
        const size_t per = (size_t)wlay_of(E, nconv, bwd).total * sizeof(float), fixed = (size_t)y.L.np * sizeof(float);
        const int cap = wide ? NPAIR : NW;
        int w = (int)((LDS_CU - fixed) / per);
        w = w < 1 ? 1 : (w > cap ? cap : w);
        lds = fixed + w * per;
        return w;
    };
    y.W_fwd = waves(false, y.lds_fwd);
    if (!wide) y.W_bwd = waves(true, y.lds_bwd);
    if (y.lds_fwd > (size_t)LDS_CU || y.lds_bwd > (size_t)LDS_CU) return fail(fn, "internal: the LDS layout does not fit");
    y.ntiles_fwd = (pl->rows + y.W_fwd - 1) / y.W_fwd;
    y.nblocks_fwd = gmpe::resident_grid(y.ntiles_fwd, y.lds_fwd, 4);
    if (wide) return GMPE_OK;
    y.ntiles_bwd = (pl->rows + y.W_bwd - 1) / y.W_bwd;
    y.nblocks_bwd = gmpe::resident_grid(y.ntiles_bwd, y.lds_bwd, 1);        // the backward kernels keep a thread's sums in registers: one wave per SIMD
    y.dX = (size_t)y.nblocks_bwd * y.L.np * sizeof(double);
    y.total = y.dX + (size_t)pl->rows * E * C * sizeof(float);
    return GMPE_OK;
}

// `table`: the plan is a gmpe_gnn_table_plan's base — node_obs and adj are not read, and agent_id is needed whatever the aggregate: the view needs its ego
int check_plan(const char* fn, const gmpe_gnn_plan* pl, bool backward, Layout& y, bool table = false, int maxe = MAXE) {
    if (int rc = check_shape(fn, pl, y, maxe)) return rc;
    const auto act = [&](const char* name, int v) {
        return v == GMPE_GNN_RELU || v == GMPE_GNN_TANH ? (int)GMPE_OK : fail(fn, std::string(name) + " must be GMPE_GNN_RELU or GMPE_GNN_TANH");
    };
    if (int rc = act("embed_activation", pl->embed_activation)) return rc;
    if (int rc = act("conv_activation", pl->conv_activation)) return rc;
    if (pl->embed_layer_norm != 0 && pl->embed_layer_norm != 1) return fail(fn, "embed_layer_norm must be 0 or 1");
    if (pl->aggregate < GMPE_GNN_NODE || pl->aggregate > GMPE_GNN_ADD) return fail(fn, "aggregate must be GMPE_GNN_NODE, _MEAN, _MAX or _ADD");
    if (!(pl->max_edge_dist == pl->max_edge_dist)) return fail(fn, "max_edge_dist must be a number");
    if (pl->embed_layer_norm && !(pl->ln_eps > 0.0)) return fail(fn, "ln_eps must be > 0");
    const bool ln = pl->embed_layer_norm != 0;
    const gmpe::PtrField top[] = {
        {table ? nullptr : pl->node_obs, "node_obs", !table}, {table ? nullptr : pl->adj, "adj", !table},
        {pl->agent_id, "agent_id", table || pl->aggregate == GMPE_GNN_NODE},
        {pl->entity_embed, "entity_embed", true}, {pl->lin1_weight, "lin1_weight", true}, {pl->lin1_bias, "lin1_bias", true},
        {pl->ln_weight, "ln_weight", ln}, {pl->ln_bias, "ln_bias", ln},
        {pl->grad_entity_embed, "grad_entity_embed", backward}, {pl->grad_lin1_weight, "grad_lin1_weight", backward},
        {pl->grad_lin1_bias, "grad_lin1_bias", backward}, {pl->grad_ln_weight, "grad_ln_weight", backward && ln}, {pl->grad_ln_bias, "grad_ln_bias", backward && ln},
        {pl->features, "features", !backward}, {pl->grad_features, "grad_features", backward}};
    if (int rc = gmpe::check_ptrs(fn, top)) return rc;
    if (((uintptr_t)pl->grad_features & 15) && backward) return fail(fn, "grad_features must be 16-byte aligned");
    for (int l = 0; l < pl->embed_layer_n; ++l) {
        const std::string n = "[" + std::to_string(l) + "]";
        if (int rc = gmpe::check_ptr(fn, pl->embed_weight[l], "embed_weight" + n, true)) return rc;
        if (int rc = gmpe::check_ptr(fn, pl->embed_bias[l], "embed_bias" + n, true)) return rc;
        if (int rc = gmpe::check_ptr(fn, pl->grad_embed_weight[l], "grad_embed_weight" + n, backward)) return rc;
        if (int rc = gmpe::check_ptr(fn, pl->grad_embed_bias[l], "grad_embed_bias" + n, backward)) return rc;
    }
    for (int c = 0; c <= pl->gnn_layer_n; ++c) {
        const gmpe_gnn_conv& v = pl->conv[c];
        const std::string n = "conv[" + std::to_string(c) + "].";
        const gmpe::PtrField fs[] = {
            {v.query_weight, "query_weight", true}, {v.query_bias, "query_bias", true}, {v.key_weight, "key_weight", true}, {v.key_bias, "key_bias", true},
            {v.value_weight, "value_weight", true}, {v.value_bias, "value_bias", true}, {v.edge_weight, "edge_weight", true},
            {v.skip_weight, "skip_weight", true}, {v.skip_bias, "skip_bias", true},
            {v.grad_query_weight, "grad_query_weight", backward}, {v.grad_query_bias, "grad_query_bias", backward},
            {v.grad_key_weight, "grad_key_weight", backward}, {v.grad_key_bias, "grad_key_bias", backward},
            {v.grad_value_weight, "grad_value_weight", backward}, {v.grad_value_bias, "grad_value_bias", backward},
            {v.grad_edge_weight, "grad_edge_weight", backward}, {v.grad_skip_weight, "grad_skip_weight", backward}, {v.grad_skip_bias, "grad_skip_bias", backward}};
        if (int rc = gmpe::check_ptrs(fn, fs, n)) return rc;
    }
    return gmpe::check_workspace(fn, pl->workspace, pl->workspace_bytes, y.total, backward, "workspace is required", "gmpe_gnn_workspace_bytes(plan, 1)");
}

GnnArgs bind(const gmpe_gnn_plan* pl, const Layout& y, bool backward) {
    GnnArgs a = {};
    a.rows = pl->rows; a.W = backward ? y.W_bwd : y.W_fwd; a.ntiles = backward ? y.ntiles_bwd : y.ntiles_fwd; a.nblocks = y.nblocks_bwd;
    a.E = pl->num_nodes; a.F = pl->node_feats; a.S = pl->adj_share; a.H = pl->heads; a.nconv = pl->gnn_layer_n + 1; a.nel = pl->embed_layer_n;
    a.eact = pl->embed_activation; a.cact = pl->conv_activation; a.ln = pl->embed_layer_norm; a.aggr = pl->aggregate;
    a.nemb = pl->num_embeddings; a.esz = pl->embedding_size; a.K1 = y.K1;
    a.maxd = (float)pl->max_edge_dist; a.lneps = (float)pl->ln_eps;
    a.x = pl->node_obs; a.adj = pl->adj; a.id = pl->agent_id;
    a.emb = pl->entity_embed; a.w1 = pl->lin1_weight; a.b1 = pl->lin1_bias; a.lnw = pl->ln_weight; a.lnb = pl->ln_bias;
    a.gemb = pl->grad_entity_embed; a.gw1 = pl->grad_lin1_weight; a.gb1 = pl->grad_lin1_bias; a.glnw = pl->grad_ln_weight; a.glnb = pl->grad_ln_bias;
    for (int l = 0; l < MAXL; ++l) {
        a.wl[l] = pl->embed_weight[l]; a.bl[l] = pl->embed_bias[l]; a.gwl[l] = pl->grad_embed_weight[l]; a.gbl[l] = pl->grad_embed_bias[l];
    }
    for (int c = 0; c < a.nconv; ++c) {
        const gmpe_gnn_conv& v = pl->conv[c];
        a.cv[c] = ConvPtr{v.query_weight, v.query_bias, v.key_weight, v.key_bias, v.value_weight, v.value_bias, v.edge_weight, v.skip_weight, v.skip_bias,
                          v.grad_query_weight, v.grad_query_bias, v.grad_key_weight, v.grad_key_bias, v.grad_value_weight, v.grad_value_bias,
                          v.grad_edge_weight, v.grad_skip_weight, v.grad_skip_bias};
    }
    a.out = pl->features; a.gout = pl->grad_features;
    a.part = static_cast<double*>(pl->workspace);
    a.dX = gmpe::at<float>(pl->workspace, y.dX);
    return a;
}

// The table plan's own fields, before its base's checks -> base, the plan the shared checks and bind() read: adj_share is not the table plan's to give
int check_table_plan(const char* fn, const gmpe_gnn_table_plan* tp, bool backward, Layout& y, gmpe_gnn_plan& base, int maxe = MAXE) {
    if (!tp) return fail(fn, "null plan");
    if (!tp->cfg) return fail(fn, "cfg is required");
    if (!tp->table) return fail(fn, "table is required");
    const gmpe_config* cfg = tp->cfg;
    if (cfg->abi_version != GMPE_ABI_VERSION) return fail(fn, "cfg.abi_version mismatch");
    const int A = cfg->num_agents, L = cfg->num_landmarks, E = gmpe_num_entities(cfg);
    if (A < 1 || A > GMPE_MAX_AGENTS || L < A || cfg->num_obstacles < 0 || E > GMPE_MAX_ENTITIES) return fail(fn, "cfg out of range");
    if (tp->base.num_nodes != E) return fail(fn, "num_nodes = " + std::to_string(tp->base.num_nodes) + " but cfg has " + std::to_string(E) + " entities");
    if (tp->base.node_feats != gmpe_node_feats(cfg))
        return fail(fn, "node_feats = " + std::to_string(tp->base.node_feats) + " but cfg's node rows have " + std::to_string(gmpe_node_feats(cfg)));
    if ((uintptr_t)tp->table & 7) return fail(fn, "table must be 8-byte aligned");
    if (tp->index64 != 0 && tp->index64 != 1) return fail(fn, "index64 must be 0 or 1");
    if ((uintptr_t)tp->table_index & (tp->index64 ? 7 : 3)) return fail(fn, tp->index64 ? "table_index must be 8-byte aligned" : "table_index must be 4-byte aligned");
    if (tp->table_rows < 1) return fail(fn, "table_rows must be >= 1");
    if (!tp->table_index) {
        if (tp->table_share < 1) return fail(fn, "table_share must be >= 1 without a table_index");
        if (tp->base.rows % tp->table_share) return fail(fn, "rows must be a multiple of table_share without a table_index");
    }
    base = tp->base;
    base.adj_share = 1;
    return check_plan(fn, &base, backward, y, true, maxe);
}

GnnTableArgs bind_table(const gmpe_gnn_table_plan* tp, const gmpe_gnn_plan& base, const Layout& y, bool backward) {
    GnnTableArgs a = {};
    static_cast<GnnArgs&>(a) = bind(&base, y, backward);
    const gmpe_config* cfg = tp->cfg;
    a.x = nullptr; a.adj = nullptr;
    a.tab = tp->table; a.tidx = tp->table_index; a.tlast = tp->table_rows - 1;
    a.idx64 = tp->index64; a.tshare = tp->table_index ? 1 : tp->table_share;
    a.kind = cfg->graph_feat_type == 1 ? 2 : (cfg->scenario >= GMPE_SCENARIO_ROT_INV ? 1 : 0);      // as gmpe_expand_node_obs picks its row kernel
    a.two = cfg->scenario == GMPE_SCENARIO_TWO_PHASE;
    a.A = cfg->num_agents; a.NL = cfg->num_landmarks; a.TW = gmpe_entity_table_width(cfg);
    return a;
}

// The launches of a checked plan, ARGS the including file's source: forward's one, backward's three
template <class ARGS>
int launch_forward(int device, const Layout& y, const ARGS& a, void* stream) {
    GMPE_HIP_CHECK(hipSetDevice(device));
    if (int rc = gmpe::raise_dynamic_lds_once(reinterpret_cast<const void*>(k_gnn_fwd<ARGS>), device, 0, LDS_CU)) return rc;
    GMPE_LAUNCH(k_gnn_fwd<ARGS>, dim3((unsigned)y.nblocks_fwd), dim3(BLOCK), y.lds_fwd, static_cast<hipStream_t>(stream), a);
    return GMPE_OK;
}
template <class ARGS>
int launch_backward(int device, const Layout& y, const ARGS& a, void* stream) {
    GMPE_HIP_CHECK(hipSetDevice(device));
    if (int rc = gmpe::raise_dynamic_lds_once(reinterpret_cast<const void*>(k_gnn_bwd_conv<ARGS>), device, 1, LDS_CU)) return rc;
    if (int rc = gmpe::raise_dynamic_lds_once(reinterpret_cast<const void*>(k_gnn_bwd_embed<ARGS>), device, 2, LDS_CU)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const GnnArgs& base = a;
    GMPE_LAUNCH(k_gnn_bwd_conv<ARGS>, dim3((unsigned)y.nblocks_bwd), dim3(BLOCK), y.lds_bwd, st, a);
    GMPE_LAUNCH(k_gnn_bwd_embed<ARGS>, dim3((unsigned)y.nblocks_bwd), dim3(BLOCK), y.lds_bwd, st, a);
    GMPE_LAUNCH(k_gnn_finish, dim3((unsigned)((y.L.np + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, base);
    return GMPE_OK;
}

}  // namespace
