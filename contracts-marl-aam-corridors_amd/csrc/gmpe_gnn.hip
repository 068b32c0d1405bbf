// gmpe_gnn.hip — the policy's GNNBase from node rows and a dense adjacency (include/gmpe.h gmpe_gnn_forward / gmpe_gnn_backward): the entry points, and
// the kernels of gmpe_gnn_kernels.h instantiated over that source. The mapping, the arithmetic and the host checks are written there; the geometry here.
// gmpe_gnn_table.hip includes this file with GMPE_GNN_TABLE defined: the same geometry and kernels, its own entry points in place of these.
#include "gmpe_host.h"          // include/gmpe.h, for the sizes below

namespace {

constexpr int C = GMPE_GNN_HIDDEN, BLOCK = 256, NW = BLOCK / 64;
constexpr int MAXE = GMPE_GNN_MAX_NODES, MAXH = GMPE_GNN_MAX_HEADS, MAXC = GMPE_GNN_MAX_CONVS, MAXL = GMPE_GNN_MAX_EMBED_LAYERS;
constexpr int NINS = 32;                                // row stride of a node's lin1 input in LDS: F - 1 + embedding_size <= 23 columns, zeros behind
constexpr int QDS = 40;                                 // backward's per-node row: q [16], the head's output gradient [16], max, -, 1 / sum and D (doubles), -
constexpr int LIN = C * C + C;                          // a 16 x 16 Linear with its bias

}  // namespace

#include "gmpe_gnn_kernels.h"

#ifndef GMPE_GNN_TABLE

extern "C" {

int gmpe_gnn_workspace_bytes(const gmpe_gnn_plan* plan, int32_t want_backward, size_t* bytes_out) {
    const char* fn = "gmpe_gnn_workspace_bytes";
    Layout y;
    if (int rc = gmpe::check_workspace_query(fn, bytes_out, std::string(), want_backward)) return rc;
    if (int rc = check_shape(fn, plan, y)) return rc;
    *bytes_out = want_backward ? y.total : 0;
    return GMPE_OK;
}

int gmpe_gnn_forward(int device, const gmpe_gnn_plan* pl, void* stream) {
    Layout y;
    if (int rc = check_plan("gmpe_gnn_forward", pl, false, y)) return rc;
    return launch_forward(device, y, bind(pl, y, false), stream);
}

int gmpe_gnn_backward(int device, const gmpe_gnn_plan* pl, void* stream) {
    Layout y;
    if (int rc = check_plan("gmpe_gnn_backward", pl, true, y)) return rc;
    return launch_backward(device, y, bind(pl, y, true), stream);
}

}  // extern "C"

#endif  // GMPE_GNN_TABLE
