// gmpe_gnn_wide.hip — the policy's GNNBase forward on graphs of up to 128 nodes (include/gmpe.h gmpe_gnn_forward_wide / gmpe_gnn_forward_wide_table /
// gmpe_gnn_wide_geometry), from both sources: node rows with a dense adjacency, and the fp64 entity table. Forward only: backward's per-graph state at
// 128 nodes is more LDS than a CU has. Up to 64 nodes the entries hand the plan to the narrow entries, whose launch it then is.
//
// Mapping. The narrow kernels give a node to a lane of one wave; here it belongs to a thread of a PAIR of waves. A workgroup of 256 threads owns tiles
// of W graphs, W = 2 where two graphs' state (wlay_of, the narrow forward's layout) fits the LDS next to the parameters and 1 above; pair p (waves 2p,
// 2p + 1) owns graph p of the tile and its thread t = 0 .. 127 node t. The pair shares the graph's LDS block. The masked matrix is staged by all
// threads that have the block: the pair's 128 at W = 2, all 256 at W = 1, where the second pair does nothing else. Every loop bound is the same in every
// wave, so every barrier is a uniform workgroup barrier; a pair without a graph computes nothing.
//
// The arithmetic is gmpe_gnn_kernels.h's graph_forward<false> and graph_output, the code k_gnn_fwd runs, with this mapping in place of a wave's lanes: a
// node's sums over its incoming edges run ascending in its own thread and skip what the mask excludes, heads are added ascending, a pool adds the nodes
// ascending in one thread per channel. So a node's chain of operations does not know how many threads the graph has, and a graph of <= 64 nodes padded
// with isolated ones keeps k_gnn_fwd's bits in every original node.
#include "gmpe_gnn_kernels.h"

namespace {

template <class ARGS>
__global__ __launch_bounds__(BLOCK) void k_gnn_fwd_wide(ARGS p) {
    extern __shared__ __attribute__((aligned(16))) float sh[];
    const int tid = threadIdx.x;
    const bool two = p.W == NPAIR;
    const int pair = two ? tid / PAIR : 0;              // the graph of the tile whose block this thread stages into
    const int s = two ? tid % PAIR : tid, ns = two ? PAIR : BLOCK;
    const int node = tid % PAIR;
    const bool owner = two || tid < PAIR;               // at W = 1 the second pair stages and waits
    const Lay L = lay_of(p.nemb, p.esz, p.K1, p.H, p.nconv, p.nel);
    const WLay WL = wlay_of(p.E, p.nconv, false);
    float* wl = sh + L.np + pair * WL.total;
    load_params(p, L, sh, tid);
    __syncthreads();
    for (int64_t tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
        const int64_t g = tile * p.W + pair;
        const bool active = g < p.rows;
        float x[C];
        graph_forward<false>(p, L, WL, sh, wl, s, ns, node, owner, g, active, x);
        if (active && owner && node < C) graph_output(p, wl + WL.xs, node, g);
        __syncthreads();                                // the next tile overwrites the pairs' state
    }
}

// the wide launch of a checked plan of more than MAXE nodes (check_shape's forward geometry is then a graph per pair)
template <class ARGS>
int launch_wide(int device, const Layout& y, const ARGS& a, int slot, void* stream) {
    GMPE_HIP_CHECK(hipSetDevice(device));
    if (int rc = gmpe::raise_dynamic_lds_once(reinterpret_cast<const void*>(k_gnn_fwd_wide<ARGS>), device, slot, LDS_CU)) return rc;
    GMPE_LAUNCH(k_gnn_fwd_wide<ARGS>, dim3((unsigned)y.nblocks_fwd), dim3(BLOCK), y.lds_fwd, static_cast<hipStream_t>(stream), a);
    return GMPE_OK;
}

}  // namespace

extern "C" {

int gmpe_gnn_wide_geometry(const gmpe_gnn_plan* plan, int64_t* out) {
    const char* fn = "gmpe_gnn_wide_geometry";
    Layout y;
    if (!out) return fail(fn, "out is required");
    if (int rc = check_shape(fn, plan, y, WIDE_MAXE)) return rc;
    out[0] = y.W_fwd; out[1] = (int64_t)y.lds_fwd; out[2] = y.nblocks_fwd;
    return GMPE_OK;
}

int gmpe_gnn_forward_wide(int device, const gmpe_gnn_plan* pl, void* stream) {
    Layout y;
    if (int rc = check_plan("gmpe_gnn_forward_wide", pl, false, y, false, WIDE_MAXE)) return rc;
    if (pl->num_nodes <= MAXE) return gmpe_gnn_forward(device, pl, stream);
    return launch_wide(device, y, bind(pl, y, false), 0, stream);
}

int gmpe_gnn_forward_wide_table(int device, const gmpe_gnn_table_plan* tp, void* stream) {
    Layout y;
    gmpe_gnn_plan base;
    if (int rc = check_table_plan("gmpe_gnn_forward_wide_table", tp, false, y, base, WIDE_MAXE)) return rc;
    if (base.num_nodes <= MAXE) return gmpe_gnn_forward_table(device, tp, stream);
    return launch_wide(device, y, bind_table(tp, base, y, false), 1, stream);
}

}  // extern "C"
