// gmpe_gnn.hip — the policy's GNNBase from node rows and a dense adjacency (include/gmpe.h gmpe_gnn_forward / gmpe_gnn_backward): the entry points, and
// the kernels of gmpe_gnn_kernels.h instantiated over that source. The geometry, the mapping, the arithmetic and the host checks are written there.
#include "gmpe_gnn_kernels.h"

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
