// gmpe_gnn_table.hip — the policy's GNNBase straight from the fp64 entity table (include/gmpe.h gmpe_gnn_forward_table / gmpe_gnn_backward_table): the
// entry points, and the kernels of gmpe_gnn_kernels.h instantiated over the table source. Graph g is the view of ego agent_id[g] of one table row: its matrix
// and its node rows are rebuilt in the graph's staging step with gmpe_expand.h's arithmetic, the bits gmpe_expand_adj and gmpe_expand_node_obs give, so
// neither array exists in memory. Everything behind that step is gmpe_gnn.hip's code, and a file of its own only because of the registers (see
// gmpe_gnn_kernels.h).
#define GMPE_GNN_TABLE          // gmpe_gnn.hip's geometry and gmpe_gnn_kernels.h, without gmpe_gnn.hip's entry points
#include "gmpe_gnn.hip"

namespace {

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

}  // namespace

#ifndef GMPE_GNN_WIDE           // gmpe_gnn_wide.hip includes this file for the table plan's checks and binding, with its own entry points

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

#endif  // GMPE_GNN_WIDE
