"""What the tests of the policy's GNNBase (include/gmpe.h gmpe_gnn_forward / gmpe_gnn_backward, gmpe.gnn_base) share.

The truth is a plain-torch restatement of GNNBase.forward (onpolicy/algorithms/utils/gnn_new.py:492-510, TransformerConv as in PyG 2.3.1) over the
process_adj EDGE LIST with index_add / scatter_reduce — a second formulation next to the kernels' dense loops — run in float64 with torch autograd; the
same code in float32 on the CPU gives err_ref. torch_geometric is not needed; the modules below carry the reference's attribute names and state-dict keys,
so the shipped weights of tests/golden/gnn_base.npz load into them and gmpe.gnn_base reads them as it reads the reference's GNNBase.

The accuracy rule is gru_lib's, unchanged: err(a) = max|a - a64| / max(1, max|a64|), err_dev <= 4 * err_ref + 2^-23 per array, err_ref capped at 1e-5.
"""
import functools
import os

import numpy as np
import torch
import torch.nn as nn

from gru_lib import CAP, FLOOR, bound, err  # noqa: F401  (the rule, shared)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = 16                          # GMPE_GNN_HIDDEN
MARGIN = 1e-5                   # a ReLU graph is redrawn when its smallest |pre-activation| in the float64 truth is below this
SIDE, MAX_EDGE_DIST = 2.4, 1.0

# ---------------------------------------------------------------------------------------------- the launch geometry, restated (csrc/gmpe_gnn_kernels.h)
BLOCK, NW, NINS, QDS, LIN, MAX_CU, LDS_CU = 256, 4, 32, 40, C * C + C, 256, 160 * 1024


def n_params(F, heads, gnn_n, embed_n, nemb, esz):
    """floats of a workgroup's parameter row (Lay::np)"""
    K1 = F - 1 + esz + 1
    return ((nemb * esz + 3) & ~3) + C * K1 + 3 * C + embed_n * LIN + (gnn_n + 1) * (3 * heads * LIN + heads * C + LIN)


def wave_floats(E, nconv, backward):
    r4 = lambda v: (v + 3) & ~3
    n = r4(E * (E | 1)) + E * NINS + E * C + (nconv + 1 if backward else 1) * E * C + E * 2 * C
    return n + (E * QDS + 4 * E * C if backward else 0)


def geometry(rows, E, F=7, heads=3, gnn_n=2, embed_n=1, nemb=4, esz=2):
    """W (graphs side by side in a workgroup), tiles and workgroups of the forward launch and of backward's first two, and the workspace bytes"""
    npar = n_params(F, heads, gnn_n, embed_n, nemb, esz)
    g = dict(np=npar)
    for name, bwd in (("fwd", False), ("bwd", True)):
        per, fixed = 4 * wave_floats(E, gnn_n + 1, bwd), 4 * npar
        W = max(1, min(NW, (LDS_CU - fixed) // per))
        lds = fixed + W * per
        tiles = (rows + W - 1) // W
        cap = MAX_CU * (1 if bwd else max(1, min(4, LDS_CU // lds)))
        g.update({"W_" + name: W, "lds_" + name: lds, "tiles_" + name: tiles, "blocks_" + name: min(tiles, cap)})
    g["workspace"] = g["blocks_bwd"] * npar * 8 + rows * E * C * 4
    return g


# ---------------------------------------------------------------------------------------------- the modules, with the reference's names
class EmbedLayer(nn.Module):
    def __init__(self, input_dim, num_embeddings, embedding_size, hidden, layer_N, use_ReLU, use_layerNorm, add_self_loop=False, edge_dim=1):
        super().__init__()
        self._layer_N, self._add_self_loops = layer_N, add_self_loop
        self.active_func = nn.ReLU() if use_ReLU else nn.Tanh()
        self.layer_norm = nn.LayerNorm(hidden) if use_layerNorm else nn.Identity()
        self.entity_embed = nn.Embedding(num_embeddings, embedding_size)
        self.lin1 = nn.Linear(input_dim + embedding_size + edge_dim, hidden)
        self.layers = nn.ModuleList()
        for _ in range(layer_N):
            self.layers.append(nn.Linear(hidden, hidden))
            self.layers.append(self.active_func)
            self.layers.append(self.layer_norm)


class Conv(nn.Module):
    """the parameters of a TransformerConv(16, 16, heads, concat=False, beta=False, edge_dim=1, root_weight=True)"""

    def __init__(self, heads, concat=False, beta=False):
        super().__init__()
        self.heads, self.out_channels, self.concat, self.beta, self.dropout, self.lin_beta = heads, C, concat, beta, 0.0, None
        self.lin_key, self.lin_query, self.lin_value = nn.Linear(C, heads * C), nn.Linear(C, heads * C), nn.Linear(C, heads * C)
        self.lin_edge = nn.Linear(1, heads * C, bias=False)
        self.lin_skip = nn.Linear(C, C)


class ConvNet(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.num_heads, self.concat_heads, self.edge_dim, self.max_edge_dist = cfg["heads"], False, 1, MAX_EDGE_DIST
        self.graph_aggr = "node" if cfg["aggr"] == "node" else "global"
        self.global_aggr_type = cfg["aggr"] if cfg["aggr"] != "node" else "mean"
        self.embed_layer = EmbedLayer(cfg["F"] - 1, cfg["nemb"], cfg["esz"], C, cfg["embed_n"], cfg["eact"] == "ReLU", bool(cfg["ln"]))
        self.gnn1 = Conv(cfg["heads"])
        self.gnn2 = nn.ModuleList(Conv(cfg["heads"]) for _ in range(cfg["gnn_n"]))
        self.activation = nn.ReLU() if cfg["cact"] == "ReLU" else nn.Tanh()


class Base(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.gnn = ConvNet(cfg)


SHIPPED = dict(F=7, heads=3, gnn_n=2, embed_n=1, eact="ReLU", cact="ReLU", ln=1, nemb=4, esz=2)


def config(weights="actor", **over):
    """weights: 'actor' / 'critic' (the shipped airtaxi checkpoints, F = 7), 'rotate' (the shipped F = 8 actor) or 'random'"""
    cfg = dict(SHIPPED, weights=weights, aggr="mean" if weights == "critic" else "node")
    if weights == "rotate":
        cfg["F"] = 8
    cfg.update(over)
    return cfg


def cfg_key(cfg):
    return "%s_F%d_h%d_g%d_e%d_%s_%s_ln%d_%s" % (cfg["weights"], cfg["F"], cfg["heads"], cfg["gnn_n"], cfg["embed_n"], cfg["eact"], cfg["cact"], cfg["ln"],
                                                   cfg["aggr"])


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "gnn_base.npz")))


def build(cfg, dtype=torch.float32):
    """the module of a configuration on the CPU: the shipped weights, or seeded random ones (weights U(-1, 1) / sqrt(fan_in) * 1.5, biases and the
    LayerNorm's 0.1 N(0, 1) around 0 and 1, the embedding N(0, 1))"""
    base = Base(cfg)
    if cfg["weights"] == "random":
        g = torch.Generator().manual_seed(4000 + sum(ord(c) for c in cfg_key(cfg)))
        with torch.no_grad():
            for name, p in base.named_parameters():
                if name.endswith("layer_norm.weight"):
                    p.copy_(1 + 0.1 * torch.randn(p.shape, generator=g))
                elif name.endswith("entity_embed.weight"):
                    p.copy_(torch.randn(p.shape, generator=g))
                elif p.dim() == 2:
                    p.copy_((2 * torch.rand(p.shape, generator=g) - 1) * 1.5 / max(1, p.shape[1]) ** 0.5)
                else:
                    p.copy_(0.1 * torch.randn(p.shape, generator=g))
    else:
        G = golden()
        sd = {k[len(cfg["weights"]) + 1 + len("gnn_base."):]: torch.from_numpy(v) for k, v in G.items() if k.startswith(cfg["weights"] + ".")}
        base.load_state_dict(sd, strict=True)
    return base.to(dtype)


def param_names(base):
    """the distinct parameters (the shared LayerNorm once), by state-dict name"""
    return [n for n, _ in base.named_parameters()]


# ---------------------------------------------------------------------------------------------- the restatement
def process_adj(adj, max_edge_dist):
    """TransformerConvNet.process_adj for [B, E, E]: source = row, target = column, batched node indices"""
    mask = (adj < max_edge_dist) & (adj > 0)
    idx = (adj * mask.to(adj.dtype)).nonzero(as_tuple=False)
    attr = adj[idx[:, 0], idx[:, 1], idx[:, 2]]
    off = idx[:, 0] * adj.shape[1]
    return torch.stack([off + idx[:, 1], off + idx[:, 2]], 0), attr.unsqueeze(1)


def _conv(conv, x, src, tgt, e, n, pre):
    H = conv.heads
    q, k, v = (lin(x).view(n, H, C) for lin in (conv.lin_query, conv.lin_key, conv.lin_value))
    ee = conv.lin_edge(e).view(-1, H, C)
    kj, vj = k[src] + ee, v[src] + ee
    logit = (q[tgt] * kj).sum(-1) / C ** 0.5                                        # [edges, H]
    top = torch.full((n, H), -torch.inf, dtype=x.dtype, device=x.device).scatter_reduce(0, tgt[:, None].expand(-1, H), logit.detach(), "amax",
                                                                                         include_self=True)
    ex = (logit - top[tgt]).exp()
    den = torch.zeros((n, H), dtype=x.dtype, device=x.device).index_add(0, tgt, ex)
    alpha = ex / (den[tgt] + 1e-16)
    out = torch.zeros((n, H, C), dtype=x.dtype, device=x.device).index_add(0, tgt, alpha[:, :, None] * vj)
    z = out.mean(1) + conv.lin_skip(x)
    pre.append(("node", z))
    return z


def forward(base, node_obs, adj, agent_id, pre=None):
    """GNNBase.forward over the edge list; adj [B, E, E] (materialised). `pre` collects the pre-activations as (kind, tensor) with kind 'edge' or 'node'."""
    net, emb = base.gnn, base.gnn.embed_layer
    pre = [] if pre is None else pre
    B, E, F = node_obs.shape
    (src, tgt), e = process_adj(adj, net.max_edge_dist)
    x = node_obs.reshape(B * E, F)
    xj = x[src]
    m = torch.cat([xj[:, :-1], emb.entity_embed(xj[:, -1].long()), e], 1)
    h = emb.lin1(m)
    pre.append(("edge", h))
    h = emb.layer_norm(emb.active_func(h))
    for l in range(emb._layer_N):
        h = emb.layers[3 * l](h)
        pre.append(("edge", h))
        h = emb.layers[3 * l + 2](emb.layers[3 * l + 1](h))
    x = torch.zeros((B * E, C), dtype=h.dtype, device=h.device).index_add(0, tgt, h)
    for conv in [net.gnn1] + list(net.gnn2):
        x = net.activation(_conv(conv, x, src, tgt, e, B * E, pre))
    x = x.view(B, E, C)
    if net.graph_aggr == "node":
        return x.gather(1, agent_id.long().view(B, 1, 1).expand(-1, -1, C)).squeeze(1)
    kind = net.global_aggr_type
    return x.mean(1) if kind == "mean" else (x.max(1).values if kind == "max" else x.sum(1))


def margins(base64, node_obs, adj, agent_id):
    """per graph, the smallest |pre-activation| in front of a ReLU (inf where no ReLU sees the graph)"""
    B, E, _ = node_obs.shape
    pre = []
    with torch.no_grad():
        forward(base64, node_obs.double(), adj.double(), agent_id, pre)
        (_, tgt), _ = process_adj(adj.double(), base64.gnn.max_edge_dist)
    m = torch.full((B,), torch.inf, dtype=torch.float64)
    for kind, t in pre:
        relu = isinstance(base64.gnn.embed_layer.active_func if kind == "edge" else base64.gnn.activation, nn.ReLU)
        if not relu or t.numel() == 0:
            continue
        graph = (tgt if kind == "edge" else torch.arange(B * E)) // E
        m = m.scatter_reduce(0, graph, t.abs().min(1).values, "amin", include_self=True)
    return m


# ---------------------------------------------------------------------------------------------- inputs
def draw(rng, n, E, F):
    """n graphs: positions uniform in the square, adj = float32 distances, features N(0, 1), types in {0, 1, 2}, ego uniform in [0, E)"""
    pos = rng.uniform(0, SIDE, (n, E, 2))
    adj = np.sqrt(((pos[:, :, None, :] - pos[:, None, :, :]) ** 2).sum(-1)).astype(np.float32)
    x = rng.randn(n, E, F).astype(np.float32)
    x[:, :, F - 1] = rng.randint(0, 3, (n, E))
    return x, adj, rng.randint(0, E, (n,)).astype(np.int64)


def special_graphs(x, adj, E):
    """the edge cases inside one batch, written over graphs 0 .. 5 (needs >= 6 graphs and E >= 4): no edge at all; node 1 with exactly one incoming edge;
    a complete graph; a zeroed row and column (a done agent); an entry exactly max_edge_dist (excluded); an asymmetric matrix"""
    adj[0] = 3.0
    adj[1, :, 1] = 3.0
    adj[1, 2, 1] = 0.5
    adj[2] = 0.25 + 0.5 * np.abs(np.subtract.outer(np.arange(E), np.arange(E))) / E
    adj[3, 1, :] = 0.0
    adj[3, :, 1] = 0.0
    adj[4, 0, 1], adj[4, 1, 0] = MAX_EDGE_DIST, 0.5
    adj[5] = np.triu(adj[5]) + np.tril(np.full((E, E), 3.0, np.float32), -1)          # edges only from the lower index to the higher
    adj[5, 0, 1] = 0.5
    for g in range(6):
        np.fill_diagonal(adj[g], 0.0)
    return adj


@functools.lru_cache(maxsize=None)
def inputs(n, E, key, special=False):
    """(node_obs, adj, agent_id, gf, redrawn) of a case as CPU tensors; key = cfg_key. ReLU graphs under the margin are redrawn, graph by graph."""
    cfg = CONFIGS[key]
    rng = np.random.RandomState(7000 + 131 * n + E)
    x, adj, ids = draw(rng, n, E, cfg["F"])
    if special:
        adj = special_graphs(x, adj, E)
    gf = rng.randn(n, C).astype(np.float32)
    base64 = build(cfg, torch.float64)
    redrawn = 0
    if "ReLU" in (cfg["eact"], cfg["cact"]):
        for _ in range(50):
            bad = np.nonzero((margins(base64, torch.from_numpy(x), torch.from_numpy(adj), torch.from_numpy(ids)) < MARGIN).numpy())[0]
            if len(bad) == 0:
                break
            redrawn += len(bad)
            keep = adj[:6].copy()
            x[bad], adj[bad], ids[bad] = draw(rng, len(bad), E, cfg["F"])
            if special:
                adj[:6] = keep                          # a written graph keeps its matrix: its features and its ego are redrawn
        else:
            raise AssertionError("the margin could not be met")
    return torch.from_numpy(x), torch.from_numpy(adj), torch.from_numpy(ids), torch.from_numpy(gf), redrawn


def run(base, x, adj, ids, gf):
    """-> {'features': out, 'grad_<name>': gradient} as float64 numpy arrays, in base's dtype"""
    dt = next(base.parameters()).dtype
    base.zero_grad()
    out = forward(base, x.to(dt), adj.to(dt), ids)
    (out * gf.to(dt)).sum().backward()
    res = {"features": out.detach().double().numpy()}
    for name, p in base.named_parameters():
        res["grad_" + name] = (p.grad if p.grad is not None else torch.zeros_like(p)).double().numpy()
    return res


@functools.lru_cache(maxsize=None)
def truth(n, E, key, special=False):
    """(float64 truth, {array: err_ref of the float32 CPU run}) of a case"""
    cfg = CONFIGS[key]
    x, adj, ids, gf, _ = inputs(n, E, key, special)
    t = run(build(cfg, torch.float64), x, adj, ids, gf)
    r = run(build(cfg, torch.float32), x, adj, ids, gf)
    return t, {k: err(r[k], t[k]) for k in t}


# ---------------------------------------------------------------------------------------------- the cases
_RANDOM = [config("random", heads=1, aggr="mean"), config("random", heads=4, aggr="node"), config("random", gnn_n=0, aggr="max"),
           config("random", embed_n=0, aggr="node"), config("random", embed_n=2, aggr="mean"), config("random", eact="Tanh", cact="Tanh", aggr="add"),
           config("random", eact="Tanh", aggr="node"), config("random", ln=0, aggr="mean"), config("random", F=8, nemb=3, esz=3, aggr="node"),
           config("random", F=16, heads=4, gnn_n=2, embed_n=2, nemb=16, esz=8, aggr="mean")]
_ALL = [config("actor"), config("critic"), config("actor", aggr="max"), config("actor", aggr="add"), config("rotate")] + _RANDOM
CONFIGS = {cfg_key(c): c for c in _ALL}
ACTOR, CRITIC, ACTOR_MAX, ACTOR_ADD, ROTATE = (cfg_key(c) for c in _ALL[:5])
SHAPES = ((1, 6), (5, 6), (65, 7), (33, 20), (300, 20), (12, 64))
# (graphs, E, configuration, special graphs): actor and critic over every shape; max and add at (65, 6); the F = 8 checkpoint; the random configurations.
# Shrunk, because the float32 CPU run of the restatement itself breaks the 1e-5 cap there (the gradients of the query / key weights, which are
# cancellation noise next to the largest gradient): the critic's mean pool at E = 64 (2.6e-5 with two graphs, 6.7e-5 with twelve) runs at (12, 44),
# and the F = 8 checkpoint (9e-5 at 12 x 20) at (20, 12). E = 64 is held by the actor's gather.
CRITIC_SHAPES = SHAPES[:5] + ((12, 44),)
CASES = tuple((n, E, ACTOR, False) for (n, E) in SHAPES) + tuple((n, E, CRITIC, False) for (n, E) in CRITIC_SHAPES) + \
    ((65, 6, ACTOR_MAX, False), (65, 6, ACTOR_ADD, False), (20, 12, ROTATE, False)) + \
    tuple((9, 11, cfg_key(c), False) for c in _RANDOM) + ((12, 44, cfg_key(_RANDOM[-1]), False), (8, 9, ACTOR, True), (8, 9, CRITIC, True))


def case_id(case):
    return "%dx%d_%s%s" % (case[0], case[1], case[2], "_special" if case[3] else "")
