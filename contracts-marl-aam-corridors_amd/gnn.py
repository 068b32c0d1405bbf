"""The policy's GNNBase on the device (include/gmpe.h gmpe_gnn_forward / gmpe_gnn_backward): GNNBase.forward (onpolicy/algorithms/utils/gnn_new.py:492-510)
of one module — process_adj, the EmbedConv with its per-edge MLP, the TransformerConv layers, the gather or the pool — as one launch, its backward as
three, whatever the number of graphs, of nodes and of edges. The dense adjacency is the mask and the edge attribute; no edge list is built.

    nbd_features = gmpe.gnn_base(node_obs, adj, agent_id, self.gnn_base)        # was: self.gnn_base(node_obs, adj, agent_id)

gnn_base_from_table is the same module straight from the fp64 entity table the rows and the adjacency are pure functions of (gmpe_gnn_forward_table /
gmpe_gnn_backward_table): bit for bit gnn_base on the engine's own arrays, which are then never written.

gnn_base_wide / gnn_base_wide_from_table are the forward alone on graphs of up to 128 nodes (gmpe_gnn_forward_wide / _wide_table), for rollout and
evaluation at more entities than gnn_base, and training, take: 64.

There is no torch fallback: the arrays must be on a HIP device.
"""
import ctypes as C

import torch

from . import _layers, _lib
from .engine import _need_cuda

HIDDEN = _lib.GNN_HIDDEN                                # embed_hidden_size and gnn_hidden_size the library is built for
MAX_NODES, MAX_HEADS, MAX_GNN_LAYER_N, MAX_EMBED_LAYER_N = _lib.GNN_MAX_NODES, _lib.GNN_MAX_HEADS, _lib.GNN_MAX_CONVS - 1, _lib.GNN_MAX_EMBED_LAYERS
WIDE_MAX_NODES = _lib.GNN_WIDE_MAX_NODES                # the forward-only gnn_base_wide / gnn_base_wide_from_table
MAX_FEATS, MAX_EMBEDDINGS, MAX_EMBEDDING_SIZE = _lib.GNN_MAX_FEATS, _lib.GNN_MAX_EMBEDDINGS, _lib.GNN_MAX_EMBEDDING_SIZE
_ACTIVATIONS = {"ReLU": _lib.GNN_RELU, "Tanh": _lib.GNN_TANH}
_AGGREGATES = {"mean": _lib.GNN_MEAN, "max": _lib.GNN_MAX, "add": _lib.GNN_ADD}
_CONV_LINEARS = (("lin_query", "query"), ("lin_key", "key"), ("lin_value", "value"))


def _tensor(obj, path, attr):
    return _layers.tensor_attr(obj, "base." + path, attr)


def _activation(obj, path):
    name = type(obj).__name__
    if name not in _ACTIVATIONS:
        raise NotImplementedError("base.%s is %s: gnn_base is built for ReLU and Tanh" % (path, name))
    return _ACTIVATIONS[name]


def _conv_params(conv, path, names, ps):
    """one TransformerConv, duck-typed -> its heads; appends its nine tensors in gmpe_gnn_conv's order"""
    if bool(getattr(conv, "concat", False)):
        raise NotImplementedError("base.%s.concat is set: gnn_base is built for averaged heads (gnn_concat_heads = False)" % path)
    if bool(getattr(conv, "beta", False)) or getattr(conv, "lin_beta", None) is not None:
        raise NotImplementedError("base.%s.beta is set: gnn_base is built for beta = False" % path)
    if float(getattr(conv, "dropout", 0.0)) != 0.0:
        raise NotImplementedError("base.%s.dropout = %g: gnn_base is built for dropout = 0" % (path, float(conv.dropout)))
    for attr in ("lin_query", "lin_key", "lin_value", "lin_edge", "lin_skip"):
        if getattr(conv, attr, None) is None:
            raise ValueError("base.%s.%s is missing: a TransformerConv with edge_dim = 1 and root_weight = True is expected" % (path, attr))
    if getattr(conv.lin_edge, "bias", None) is not None:
        raise ValueError("base.%s.lin_edge has a bias: TransformerConv's lin_edge has none" % path)
    for attr, short in _CONV_LINEARS:
        ps += [_tensor(getattr(conv, attr), "%s.%s" % (path, attr), "weight"), _tensor(getattr(conv, attr), "%s.%s" % (path, attr), "bias")]
        names += ["%s.%s.weight" % (path, attr), "%s.%s.bias" % (path, attr)]
    ps += [_tensor(conv.lin_edge, path + ".lin_edge", "weight"), _tensor(conv.lin_skip, path + ".lin_skip", "weight"),
           _tensor(conv.lin_skip, path + ".lin_skip", "bias")]
    names += [path + ".lin_edge.weight", path + ".lin_skip.weight", path + ".lin_skip.bias"]
    return int(getattr(conv, "heads", 1))


def _base_params(base):
    """(names, tensors, meta) of a GNNBase, duck-typed: .gnn (the TransformerConvNet) with .embed_layer (.entity_embed, .lin1, .layer_norm, .layers,
    ._layer_N, .active_func), .gnn1, .gnn2, .activation, .max_edge_dist, .graph_aggr, .global_aggr_type, .edge_dim. The tensors' order: entity_embed, lin1
    weight and bias, [LayerNorm weight and bias], (weight, bias) per embed layer, then nine per conv. A LayerNorm that the state dict names twice
    (embed_layer.layer_norm and embed_layer.layers.2) is one module, read once.
    meta = (heads, gnn_layer_N, embed_layer_N, embed activation, conv activation, layer norm, ln eps, aggregate, max_edge_dist)."""
    net = getattr(base, "gnn", None)
    emb = getattr(net, "embed_layer", None)
    if net is None or emb is None or getattr(net, "gnn1", None) is None:
        raise ValueError("base must have .gnn with .embed_layer, .gnn1 and .gnn2: the reference's GNNBase")
    if int(getattr(net, "edge_dim", 1)) != 1:
        raise NotImplementedError("edge_dim = %d: gnn_base is built for edge_dim = 1" % int(net.edge_dim))
    embed_n = int(getattr(emb, "_layer_N", 0))
    if embed_n < 0:
        raise ValueError("base.gnn.embed_layer._layer_N = %d must be >= 0" % embed_n)
    if embed_n > MAX_EMBED_LAYER_N:
        raise NotImplementedError("embed_layer_N = %d: gnn_base is built for embed_layer_N in 0 .. %d" % (embed_n, MAX_EMBED_LAYER_N))
    layers = getattr(emb, "layers", ()) if embed_n else ()
    if embed_n and len(layers) < 3 * embed_n:
        raise ValueError("base.gnn.embed_layer.layers holds %d modules, fewer than 3 * embed_layer_N = %d" % (len(layers), 3 * embed_n))
    gnn2 = getattr(net, "gnn2", ())
    gnn_n = len(gnn2)
    if gnn_n > MAX_GNN_LAYER_N:
        raise NotImplementedError("gnn_layer_N = %d: gnn_base is built for gnn_layer_N in 0 .. %d" % (gnn_n, MAX_GNN_LAYER_N))
    names, ps = ["embed_layer.entity_embed.weight", "embed_layer.lin1.weight", "embed_layer.lin1.bias"], [
        _tensor(emb.entity_embed, "gnn.embed_layer.entity_embed", "weight"), _tensor(emb.lin1, "gnn.embed_layer.lin1", "weight"),
        _tensor(emb.lin1, "gnn.embed_layer.lin1", "bias")]
    norm = getattr(emb, "layer_norm", None)
    ln = isinstance(getattr(norm, "weight", None), torch.Tensor)                    # nn.Identity has none
    ln_eps = float(getattr(norm, "eps", 1e-5)) if ln else 1e-5
    if ln:
        ps += [norm.weight, _tensor(norm, "gnn.embed_layer.layer_norm", "bias")]
        names += ["embed_layer.layer_norm.weight", "embed_layer.layer_norm.bias"]
    eact = _activation(getattr(emb, "active_func", None), "gnn.embed_layer.active_func")
    for l in range(embed_n):
        lin, a, nm = layers[3 * l], layers[3 * l + 1], layers[3 * l + 2]
        if _activation(a, "gnn.embed_layer.layers[%d]" % (3 * l + 1)) != eact:
            raise NotImplementedError("gnn_base is built for one activation in every embed layer")
        if ln and nm is not norm:
            raise NotImplementedError("base.gnn.embed_layer.layers[%d] is not embed_layer.layer_norm: gnn_base is built for the one shared LayerNorm"
                                      % (3 * l + 2))
        ps += [_tensor(lin, "gnn.embed_layer.layers[%d]" % (3 * l), "weight"), _tensor(lin, "gnn.embed_layer.layers[%d]" % (3 * l), "bias")]
        names += ["embed_layer.layers.%d.weight" % (3 * l), "embed_layer.layers.%d.bias" % (3 * l)]
    heads = [_conv_params(net.gnn1, "gnn.gnn1", names, ps)] + [_conv_params(gnn2[i], "gnn.gnn2[%d]" % i, names, ps) for i in range(gnn_n)]
    if len(set(heads)) != 1:
        raise NotImplementedError("heads %s: gnn_base is built for one number of heads in every conv" % heads)
    if not 1 <= heads[0] <= MAX_HEADS:
        raise NotImplementedError("gnn_num_heads = %d: gnn_base is built for 1 .. %d heads" % (heads[0], MAX_HEADS))
    cact = _activation(getattr(net, "activation", None), "gnn.activation")
    aggr = str(getattr(net, "graph_aggr", "node"))
    if aggr == "node":
        aggregate = _lib.GNN_NODE
    elif aggr == "global":
        kind = str(getattr(net, "global_aggr_type", "mean"))
        if kind not in _AGGREGATES:
            raise ValueError("base.gnn.global_aggr_type = %r must be 'mean', 'max' or 'add'" % kind)
        aggregate = _AGGREGATES[kind]
    else:
        raise ValueError("base.gnn.graph_aggr = %r must be 'node' or 'global'" % aggr)
    return names, ps, (heads[0], gnn_n, embed_n, eact, cact, int(ln), ln_eps, aggregate, float(net.max_edge_dist))


def _check(node_obs, adj, agent_id, names, ps, meta, who="gnn_base", max_nodes=MAX_NODES):
    """Everything the host can see, before the device is touched -> (device, rows, E, F, adj_share, num_embeddings, embedding_size)"""
    for name, t in (("node_obs", node_obs), ("adj", adj), ("agent_id", agent_id)):
        if not isinstance(t, torch.Tensor):
            raise ValueError("%s must be a tensor" % name)
    tensors = [("node_obs", node_obs), ("adj", adj)] + [("base.gnn." + n, t) for n, t in zip(names, ps)]
    _layers.need_float32(who, tensors)
    if agent_id.dtype not in (torch.int32, torch.int64, torch.float32):
        raise ValueError("agent_id must be int32, int64 or float32, not %s" % agent_id.dtype)
    if node_obs.dim() != 3 or min(node_obs.shape) < 1:
        raise ValueError("node_obs must have shape (rows, E, F), not %s" % (tuple(node_obs.shape),))
    rows, E, F = (int(v) for v in node_obs.shape)
    if E > max_nodes:
        raise NotImplementedError("E = %d nodes: %s is built for at most %d" % (E, who, max_nodes))
    if not 2 <= F <= MAX_FEATS:
        raise NotImplementedError("F = %d node features: gnn_base is built for 2 .. %d" % (F, MAX_FEATS))
    if adj.dim() != 3 or adj.shape[1] != E or adj.shape[2] != E or adj.shape[0] < 1 or rows % int(adj.shape[0]):
        raise ValueError("adj must have shape (rows, E, E) or (rows / S, E, E) = (%d / S, %d, %d), not %s" % (rows, E, E, tuple(adj.shape)))
    share = rows // int(adj.shape[0])
    _check_ids(agent_id, rows)
    nemb, esz = _check_params(names, ps, meta, F)
    dev = node_obs.device
    _need_cuda(dev)
    _layers.need_device(tensors + [("agent_id", agent_id)], dev, "node_obs")
    return dev, rows, E, F, share, nemb, esz


def _check_ids(agent_id, rows):
    if agent_id.dim() == 2 and agent_id.shape[0] == rows and agent_id.shape[1] > 1:
        raise NotImplementedError("agent_id has %d ids per row: gnn_base is built for one" % agent_id.shape[1])
    if tuple(agent_id.shape) not in ((rows,), (rows, 1)):
        raise ValueError("agent_id must have shape (rows,) or (rows, 1) = (%d,), not %s" % (rows, tuple(agent_id.shape)))


def _check_params(names, ps, meta, F):
    """the parameters' shapes for F node features -> (num_embeddings, embedding_size)"""
    heads, gnn_n, embed_n, _, _, ln, _, aggregate, _ = meta
    table, w1 = ps[0], ps[1]
    if table.dim() != 2 or w1.dim() != 2:
        raise ValueError("base.gnn.embed_layer.entity_embed.weight and lin1.weight must be matrices")
    nemb, esz = (int(v) for v in table.shape)
    if int(w1.shape[0]) != HIDDEN:
        raise NotImplementedError("embed_hidden_size = %d: gnn_base is built for embed_hidden_size = gnn_hidden_size = %d" % (w1.shape[0], HIDDEN))
    if not 1 <= nemb <= MAX_EMBEDDINGS:
        raise NotImplementedError("num_embeddings = %d: gnn_base is built for 1 .. %d" % (nemb, MAX_EMBEDDINGS))
    if not 1 <= esz <= MAX_EMBEDDING_SIZE:
        raise NotImplementedError("embedding_size = %d: gnn_base is built for 1 .. %d" % (esz, MAX_EMBEDDING_SIZE))
    skip = ps[3 + 2 * ln + 2 * embed_n + 7]
    if skip.dim() == 2 and int(skip.shape[0]) != HIDDEN:
        raise NotImplementedError("gnn_hidden_size = %d: gnn_base is built for embed_hidden_size = gnn_hidden_size = %d" % (skip.shape[0], HIDDEN))
    hc = HIDDEN * heads
    shapes = [(nemb, esz), (HIDDEN, F - 1 + esz + 1), (HIDDEN,)] + [(HIDDEN,), (HIDDEN,)] * ln + [(HIDDEN, HIDDEN), (HIDDEN,)] * embed_n + \
        [(hc, HIDDEN), (hc,), (hc, HIDDEN), (hc,), (hc, HIDDEN), (hc,), (hc, 1), (HIDDEN, HIDDEN), (HIDDEN,)] * (gnn_n + 1)
    for name, t, s in zip(names, ps, shapes):
        if tuple(t.shape) != s:
            raise ValueError("base.gnn.%s must have shape %s (F = %d, %d heads of %d, averaged), not %s" % (name, s, F, heads, HIDDEN, tuple(t.shape)))
    return nemb, esz


def _shape_plan(rows, E, F, share, heads, gnn_n, embed_n, nemb, esz):
    p = _lib.GmpeGnnPlan()
    p.rows, p.num_nodes, p.node_feats, p.adj_share, p.hidden, p.heads, p.edge_dim = rows, E, F, share, HIDDEN, heads, 1
    p.gnn_layer_n, p.embed_layer_n, p.num_embeddings, p.embedding_size = gnn_n, embed_n, nemb, esz
    return p


def gnn_workspace_bytes(rows, num_nodes, node_feats, heads=3, gnn_layer_N=2, embed_layer_N=1, num_embeddings=4, embedding_size=2, backward=True):
    """Device scratch (bytes) one training gnn_base call over `rows` graphs of `num_nodes` nodes needs (gmpe_gnn_workspace_bytes); 0 without backward.
    A function of these shapes and counts alone, never of the edges."""
    for name, v, lo, hi in (("E", num_nodes, 1, MAX_NODES), ("F", node_feats, 2, MAX_FEATS), ("gnn_num_heads", heads, 1, MAX_HEADS),
                            ("gnn_layer_N", gnn_layer_N, 0, MAX_GNN_LAYER_N), ("embed_layer_N", embed_layer_N, 0, MAX_EMBED_LAYER_N),
                            ("num_embeddings", num_embeddings, 1, MAX_EMBEDDINGS), ("embedding_size", embedding_size, 1, MAX_EMBEDDING_SIZE)):
        if not lo <= int(v) <= hi:
            raise NotImplementedError("%s = %d: gnn_base is built for %s in %d .. %d" % (name, int(v), name, lo, hi))
    n = C.c_size_t()
    plan = _shape_plan(int(rows), int(num_nodes), int(node_feats), 1, int(heads), int(gnn_layer_N), int(embed_layer_N), int(num_embeddings),
                       int(embedding_size))
    _lib.check(_lib.load().gmpe_gnn_workspace_bytes(C.byref(plan), int(bool(backward)), C.byref(n)), "gmpe_gnn_workspace_bytes")
    return int(n.value)


def _fill(p, meta, ln, embed_n, gnn_n, ps, prefix):
    """the parameter (prefix '') or gradient (prefix 'grad_') pointers of a plan, from the tensors in _base_params' order"""
    it = iter(ps)
    for k in ("entity_embed", "lin1_weight", "lin1_bias") + (("ln_weight", "ln_bias") if ln else ()):
        setattr(p, prefix + k, next(it).data_ptr())
    for l in range(embed_n):
        getattr(p, prefix + "embed_weight")[l] = next(it).data_ptr()
        getattr(p, prefix + "embed_bias")[l] = next(it).data_ptr()
    for c in range(gnn_n + 1):
        for k in _lib.GNN_CONV_PARAMS:
            setattr(p.conv[c], prefix + k, next(it).data_ptr())


def _plan(shape, meta, node_obs, adj, agent_id, ps):
    heads, gnn_n, embed_n, eact, cact, ln, ln_eps, aggregate, max_dist = meta
    rows, E, F, share, nemb, esz = shape
    p = _shape_plan(rows, E, F, share, heads, gnn_n, embed_n, nemb, esz)
    p.embed_activation, p.conv_activation, p.embed_layer_norm, p.aggregate, p.max_edge_dist, p.ln_eps = eact, cact, ln, aggregate, max_dist, ln_eps
    if node_obs is not None:                            # None: the base of a table plan, which reads neither
        p.node_obs, p.adj = node_obs.data_ptr(), adj.data_ptr()
    p.agent_id = agent_id.data_ptr()
    _fill(p, meta, ln, embed_n, gnn_n, ps, "")
    return p


def _forward(name, meta, shape, node_obs, adj, agent_id, ps):
    """the forward entry `name` over the rows and the adjacency -> (features, the contiguous inputs the plan points at)"""
    dev = node_obs.device
    cs = [t.detach().contiguous() for t in (node_obs, adj, agent_id) + tuple(ps)]
    features = torch.empty((shape[0], HIDDEN), dtype=torch.float32, device=dev)
    plan = _plan(shape, meta, cs[0], cs[1], cs[2], cs[3:])
    plan.features = features.data_ptr()
    _layers.run(name, dev, plan)
    return features, cs


class _Base(torch.autograd.Function):
    """features = base(node_obs, adj, agent_id) as one node over all parameters. gmpe_gnn_backward recomputes a graph's forward, so only the inputs are
    kept; changing any of them in place before backward is the caller's error, as with any saved tensor. The workspace is backward's own scratch."""

    @staticmethod
    def forward(ctx, meta, shape, workspace, node_obs, adj, agent_id, *ps):
        features, cs = _forward("gmpe_gnn_forward", meta, shape, node_obs, adj, agent_id, ps)
        if workspace is not None:
            ctx.save_for_backward(*cs)
        ctx.meta, ctx.shape, ctx.workspace = meta, shape, workspace
        return features

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gf):
        cs = list(ctx.saved_tensors)
        dev = cs[0].device
        gf = gf.contiguous()
        grads = [torch.empty_like(t) for t in cs[3:]]
        plan = _plan(ctx.shape, ctx.meta, cs[0], cs[1], cs[2], cs[3:])              # backward neither reads nor writes features
        plan.grad_features = gf.data_ptr()
        plan.workspace, plan.workspace_bytes = ctx.workspace.data_ptr(), ctx.workspace.numel()
        _fill(plan, ctx.meta, ctx.meta[5], ctx.meta[2], ctx.meta[1], grads, "grad_")
        _layers.run("gmpe_gnn_backward", dev, plan)
        return (None, None, None, None, None, None) + tuple(grads)


def _table_plan(shape, meta, cfg, share, table, index, agent_id, ps):
    """gmpe_gnn_table_plan around _plan's base: the table [table_rows, W], the index or the share"""
    tp = _lib.GmpeGnnTablePlan()
    tp.base = _plan(shape, meta, None, None, agent_id, ps)
    tp.cfg, tp.table, tp.table_rows = C.pointer(cfg), table.data_ptr(), table.numel() // table.shape[-1]
    if index is not None:
        tp.table_index, tp.index64 = index.data_ptr(), int(index.dtype == torch.int64)
    tp.table_share = share
    return tp


def _forward_table(name, meta, shape, cfg, share, table, index, agent_id, ps):
    """the forward entry `name` over the entity table -> (features, the contiguous ids and parameters the plan points at)"""
    dev = table.device
    cs = [t.detach().contiguous() for t in (agent_id,) + tuple(ps)]
    features = torch.empty((shape[0], HIDDEN), dtype=torch.float32, device=dev)
    tp = _table_plan(shape, meta, cfg, share, table, index, cs[0], cs[1:])
    tp.base.features = features.data_ptr()
    _layers.run(name, dev, tp)
    return features, cs


class _BaseTable(torch.autograd.Function):
    """_Base with a graph's rows and matrix rebuilt from the entity table (gmpe_gnn_forward_table / _backward_table): the table, the index and the ids are
    kept in place of node_obs and adj."""

    @staticmethod
    def forward(ctx, meta, shape, workspace, cfg, share, table, index, agent_id, *ps):
        features, cs = _forward_table("gmpe_gnn_forward_table", meta, shape, cfg, share, table, index, agent_id, ps)
        if workspace is not None:
            ctx.save_for_backward(*cs)
            ctx.source = (cfg, share, table, index)
        ctx.meta, ctx.shape, ctx.workspace = meta, shape, workspace
        return features

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gf):
        cs = list(ctx.saved_tensors)
        cfg, share, table, index = ctx.source
        gf = gf.contiguous()
        grads = [torch.empty_like(t) for t in cs[1:]]
        tp = _table_plan(ctx.shape, ctx.meta, cfg, share, table, index, cs[0], cs[1:])
        tp.base.grad_features = gf.data_ptr()
        tp.base.workspace, tp.base.workspace_bytes = ctx.workspace.data_ptr(), ctx.workspace.numel()
        _fill(tp.base, ctx.meta, ctx.meta[5], ctx.meta[2], ctx.meta[1], grads, "grad_")
        _layers.run("gmpe_gnn_backward_table", table.device, tp)
        return (None,) * 8 + tuple(grads)


def gnn_base_from_table(entity_table, table_index, agent_id, base, cfg, *, table_share=None, workspace=None):
    """gnn_base(node_obs[table_index, agent_id], adj[table_index], agent_id, base) straight from the fp64 entity table those arrays are pure functions
    of (gmpe_gnn_forward_table / _backward_table) -> nbd_features [rows, 16], bit for bit gnn_base's on the engine's own rows and adjacency, in the
    output and in every parameter gradient (for equal `rows`: a parameter gradient's summation order is a function of (rows, E, configuration)).
    Neither [rows, E, F] nor [rows, E, E] is ever written: a graph costs its index next to a table that is already there. It is NOT faster than
    gnn_base on arrays that exist — the GNN's arithmetic dominates, and every graph rebuilds its own matrix —: its purpose is bytes.
    entity_table: contiguous float64 device tensor [..., W], W = cfg.entity_table_width (an engine's out.entity_table, a DeviceRolloutBuffer's
    entity_table); the leading dims are flattened to table rows. It is not copied: it must stay unchanged until backward has run.
    table_index: int32 or int64 [rows], the table row of every graph (t * N + n for a buffer's [T+1, N, W]); or None with table_share = S, where
    table row g // S serves graph g (a rollout step's [N, W] table with S = num_agents) and rows = table rows * S.
    agent_id: gnn_base's, the ego whose view graph g is; needed whatever base's aggregate. An index outside the table and an id outside
    [0, num_agents) are clamped: nothing is read out of bounds, and that row's value is unspecified.
    base, workspace: gnn_base's, with its refusals; the node features and the entity count are cfg's. One autograd node over all parameters, nothing
    saved under torch.no_grad()."""
    names, ps, meta = _base_params(base)
    rows, share, E, F, nemb, esz, dev, ids, index = _check_table(entity_table, table_index, agent_id, (names, ps, meta), cfg, table_share)
    train = torch.is_grad_enabled() and any(t.requires_grad for t in ps)
    workspace = _layers.backward_workspace(train, lambda: gnn_workspace_bytes(rows, E, F, meta[0], meta[1], meta[2], nemb, esz), workspace, dev)
    return _BaseTable.apply(meta, (rows, E, F, 1, nemb, esz), workspace, cfg, share, entity_table.detach(), index, ids, *ps)


def _check_table(entity_table, table_index, agent_id, params, cfg, table_share, who="gnn_base", max_nodes=MAX_NODES):
    """gnn_base_from_table's arguments, params = _base_params(base), before the device is touched -> (rows, table_share, E, F, num_embeddings,
    embedding_size, device, the ids as int32 [rows], the index contiguous or None)"""
    names, ps, meta = params
    if not isinstance(entity_table, torch.Tensor) or not isinstance(agent_id, torch.Tensor):
        raise ValueError("entity_table and agent_id must be tensors")
    if entity_table.dtype != torch.float64:
        raise ValueError("entity_table must be float64, not %s" % entity_table.dtype)
    W = int(cfg.entity_table_width)
    if entity_table.dim() < 2 or int(entity_table.shape[-1]) != W or entity_table.numel() < W:
        raise ValueError("entity_table must have shape (..., W) with W = cfg.entity_table_width = %d and at least one row, not %s"
                         % (W, tuple(entity_table.shape)))
    if not entity_table.is_contiguous():
        raise ValueError("entity_table must be contiguous")
    table_rows = entity_table.numel() // W
    if table_index is not None:
        if table_share is not None:
            raise ValueError("table_share is for table_index = None: give one of them")
        if not isinstance(table_index, torch.Tensor) or table_index.dtype not in (torch.int32, torch.int64):
            raise ValueError("table_index must be an int32 or int64 tensor, or None with table_share")
        if table_index.dim() != 1 or table_index.shape[0] < 1:
            raise ValueError("table_index must have shape (rows,), not %s" % (tuple(table_index.shape),))
        rows, share = int(table_index.shape[0]), 1
    else:
        if table_share is None or isinstance(table_share, bool) or int(table_share) != table_share or int(table_share) < 1:
            raise ValueError("table_index is None: table_share must be an integer >= 1, not %r" % (table_share,))
        share = int(table_share)
        rows = table_rows * share
    E, F = int(cfg.num_entities), int(cfg.node_feats)
    if E > max_nodes:
        raise NotImplementedError("E = %d nodes: %s is built for at most %d" % (E, who, max_nodes))
    _layers.need_float32(who + "_from_table", [("base.gnn." + n, t) for n, t in zip(names, ps)])
    if agent_id.dtype not in (torch.int32, torch.int64, torch.float32):
        raise ValueError("agent_id must be int32, int64 or float32, not %s" % agent_id.dtype)
    _check_ids(agent_id, rows)
    nemb, esz = _check_params(names, ps, meta, F)
    dev = entity_table.device
    _need_cuda(dev)
    others = [("agent_id", agent_id)] + ([("table_index", table_index)] if table_index is not None else [])
    _layers.need_device([("base.gnn." + n, t) for n, t in zip(names, ps)] + others, dev, "entity_table")
    ids = agent_id.detach().reshape(rows).to(torch.int32)
    index = None if table_index is None else table_index.detach().contiguous()
    return rows, share, E, F, nemb, esz, dev, ids, index


def gnn_base(node_obs, adj, agent_id, base, workspace=None):
    """GNNBase.forward(node_obs, adj, agent_id) of `base` on the device -> nbd_features [rows, 16].
    node_obs: float32 [rows, E, F], the last column the entity type; 1 <= E <= 64, 2 <= F <= 16.
    adj: float32 [rows, E, E], or [rows / S, E, E] where matrix g // S serves row g (the compact adjacency of a rollout step, S = num_agents); the result
    has the bits of the materialised form. Edge j -> i exists iff 0 < adj[j, i] < max_edge_dist; the matrix need not be symmetric.
    agent_id: [rows] or [rows, 1], int32, int64 or float32 (converted to int32); read with graph_aggr = 'node' only. An id outside [0, E) and an entity
    type outside [0, num_embeddings) are clamped: nothing is read out of bounds, and that row's value is unspecified.
    base: duck-typed — .gnn with .embed_layer (.entity_embed, .lin1, .layer_norm, .layers, ._layer_N, .active_func), .gnn1 and .gnn2[i] (each
    .lin_query / .lin_key / .lin_value / .lin_edge / .lin_skip, .heads, .concat, .beta), .activation, .max_edge_dist, .graph_aggr, .global_aggr_type.
    The reference's GNNBase works unchanged; the parameters are read from the module, so the optimiser and the checkpoints do not change. Gradients
    reach every parameter through one autograd node (three launches); the inputs are environment data and get none. Under torch.no_grad(), or when no
    parameter requires a gradient, the forward-only plan runs: no workspace, nothing saved. float32, hidden 16, 1 .. 4 averaged heads, gnn_layer_N and
    embed_layer_N in 0 .. 2, ReLU or Tanh, edge_dim 1; everything else is refused by name before any launch. embed_add_self_loop is inert in the
    reference (it tests edge_attr is None) and is ignored. Nothing here waits for the device. A graph's result does not depend on the other graphs, so
    the rows may be chunked freely.
    workspace: an optional uint8 device tensor of gnn_workspace_bytes(...) to reuse between calls — backward's scratch, so it belongs to one forward
    until that forward's backward has run."""
    names, ps, meta = _base_params(base)
    dev, rows, E, F, share, nemb, esz = _check(node_obs, adj, agent_id, names, ps, meta)
    ids = agent_id.detach().reshape(rows).to(torch.int32)
    train = torch.is_grad_enabled() and any(t.requires_grad for t in ps)
    workspace = _layers.backward_workspace(train, lambda: gnn_workspace_bytes(rows, E, F, meta[0], meta[1], meta[2], nemb, esz), workspace, dev)
    return _Base.apply(meta, (rows, E, F, share, nemb, esz), workspace, node_obs, adj, ids, *ps)


def _forward_only(ps):
    if torch.is_grad_enabled() and any(t.requires_grad for t in ps):
        raise NotImplementedError("a parameter of base requires a gradient and gradients are enabled, but gnn_base_wide is forward only: backward at "
                                  "E > %d is not built (call it under torch.no_grad(), or train with gnn_base at E <= %d)" % (MAX_NODES, MAX_NODES))


def gnn_base_wide(node_obs, adj, agent_id, base):
    """gnn_base's forward on graphs of 1 <= E <= 128 nodes (gmpe_gnn_forward_wide) -> nbd_features [rows, 16]: rollout, evaluation and the value
    bootstrap of a policy at more entities than it can be trained on here — the GNN's weights do not depend on E. The arguments, the checks and the
    parameter reader are gnn_base's. Forward only, without an autograd node: with gradients enabled and a parameter of base requiring one it raises
    NotImplementedError before any launch; under torch.no_grad(), or with frozen parameters, it runs.
    E <= 64 runs gnn_base's own launch: its bits. E > 64 runs one launch in which a node belongs to a thread of a pair of waves; a graph's arithmetic
    is the same function of E and the configuration, so a graph of <= 64 nodes padded with isolated nodes (type 0, adjacency entries 0 or >=
    max_edge_dist) keeps gnn_base's bits in every original node. A graph's result does not depend on the other graphs of the call."""
    names, ps, meta = _base_params(base)
    _forward_only(ps)
    _, rows, E, F, share, nemb, esz = _check(node_obs, adj, agent_id, names, ps, meta, "gnn_base_wide", WIDE_MAX_NODES)
    ids = agent_id.detach().reshape(rows).to(torch.int32)
    return _forward("gmpe_gnn_forward_wide", meta, (rows, E, F, share, nemb, esz), node_obs, adj, ids, ps)[0]


def gnn_base_wide_from_table(entity_table, table_index, agent_id, base, cfg, table_share=None):
    """gnn_base_wide straight from the fp64 entity table (gmpe_gnn_forward_wide_table) -> nbd_features [rows, 16], bit for bit gnn_base_wide on the
    engine's own rows and adjacency; cfg.num_entities may be up to 128. The arguments and the checks are gnn_base_from_table's; forward only, as
    gnn_base_wide."""
    names, ps, meta = _base_params(base)
    _forward_only(ps)
    rows, share, E, F, nemb, esz, _, ids, index = _check_table(entity_table, table_index, agent_id, (names, ps, meta), cfg, table_share,
                                                               "gnn_base_wide", WIDE_MAX_NODES)
    return _forward_table("gmpe_gnn_forward_wide_table", meta, (rows, E, F, 1, nemb, esz), cfg, share, entity_table.detach(), index, ids, ps)[0]


def wide_geometry(rows, num_nodes, node_feats, heads=3, gnn_layer_N=2, embed_layer_N=1, num_embeddings=4, embedding_size=2):
    """(graphs side by side in a workgroup, dynamic LDS bytes, workgroups) of the launch gnn_base_wide makes for these shapes and counts
    (gmpe_gnn_wide_geometry); no device is touched. Up to 64 nodes it is gnn_base's forward launch."""
    out = (C.c_int64 * 3)()
    plan = _shape_plan(int(rows), int(num_nodes), int(node_feats), 1, int(heads), int(gnn_layer_N), int(embed_layer_N), int(num_embeddings),
                       int(embedding_size))
    _lib.check(_lib.load().gmpe_gnn_wide_geometry(C.byref(plan), out), "gmpe_gnn_wide_geometry")
    return int(out[0]), int(out[1]), int(out[2])
