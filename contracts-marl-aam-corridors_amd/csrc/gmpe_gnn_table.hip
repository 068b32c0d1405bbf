// gmpe_gnn_table.hip — the policy's GNNBase straight from the fp64 entity table (include/gmpe.h gmpe_gnn_forward_table / gmpe_gnn_backward_table): the
// entry points, and the kernels of gmpe_gnn_kernels.h instantiated over the table source. Graph g is the view of ego agent_id[g] of one table row: its matrix
// and its node rows are rebuilt in the graph's staging step with gmpe_expand.h's arithmetic, the bits gmpe_expand_adj and gmpe_expand_node_obs give, so
// neither array exists in memory. Everything behind that step is gmpe_gnn.hip's code, and a file of its own only because of the registers (see
// gmpe_gnn_kernels.h, which also has the table plan's checks and binding).
#include "gmpe_gnn_kernels.h"

extern "C" {

int gmpe_gnn_forward_table(int device, const gmpe_gnn_table_plan* tp, void* stream) {
    Layout y;
    gmpe_gnn_plan base;
    if (int rc = check_table_plan("gmpe_gnn_forward_table", tp, false, y, base)) return rc;
    return launch_forward(device, y, bind_table(tp, base, y, false), stream);
}

int gmpe_gnn_backward_table(int device, const gmpe_gnn_table_plan* tp, void* stream) {
    Layout y;
    gmpe_gnn_plan base;
    if (int rc = check_table_plan("gmpe_gnn_backward_table", tp, true, y, base)) return rc;
    return launch_backward(device, y, bind_table(tp, base, y, true), stream);
}

}  // extern "C"
