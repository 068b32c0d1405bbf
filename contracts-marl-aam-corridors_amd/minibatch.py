"""PPO minibatches drawn on the device from a rollout's [T+1, N, ...] arrays (GraphReplayBuffer.feed_forward_generator / recurrent_generator,
onpolicy/utils/graph_buffer.py:368-758, called by GR_MAPPO.train, onpolicy/algorithms/graph_mappo.py:319-331).

One minibatch is one gmpe_minibatch_gather call (include/gmpe.h; csrc/gmpe_minibatch.hip): every field's rows are gathered through the device permutation into one
fresh slab, in the reference's shapes, dtypes and order — the 16-tuple ppo_update consumes unchanged. The arrays may be in any storage form of the rollout buffer:
node rows or the fp64 entity table, materialised [.., A, E, E] / compact [.., E, E] / no adjacency (rebuilt from the table, bit-identical to the engine). No engine
is needed, so a learner rank can run this on a ShardedRolloutCollector.unpack result or on raw entity tables.

The policy consumes an edge list, not the matrices (GNNBase.forward -> TransformerConvNet.process_adj, onpolicy/algorithms/utils/gnn_new.py:329-358, 492-510):
Gather.edges / adj="edges" emit that list for a minibatch straight from the stored adjacency form (gmpe_minibatch_edges; csrc/gmpe_mb_edges.hip), so the
[rows, E, E] batch is never written.
"""
import collections
import ctypes as C
import numbers

import torch

from . import _lib

# the reference's yield order (graph_buffer.py:461-465, 753-757); "advantages" is adv_targ, "action_log_probs" old_action_log_probs_batch
TUPLE = ("share_obs", "obs", "node_obs", "adj", "agent_id", "share_agent_id", "rnn_states", "rnn_states_critic", "actions", "value_preds", "returns", "masks",
         "active_masks", "action_log_probs", "advantages", "available_actions")
LEARNER = ("rnn_states", "rnn_states_critic", "actions", "action_log_probs")
_ALIGN = 256

# process_adj's result for one minibatch: edge_index [2, n] (row 0 sources, row 1 destinations; node ids graph * num_nodes + i), edge_attr [n, 1], and the
# true edge count n_edges — an int in the exact mode, an int32 device tensor [1] with an explicit cap (then n = cap and only min(n_edges, cap) entries are edges)
EdgeList = collections.namedtuple("EdgeList", ("edge_index", "edge_attr", "num_graphs", "num_nodes", "n_edges"))
# A minibatch's graphs addressed through the entity table the buffer already holds (adj="table"): `table` the buffer's own [T+1, N, W] tensor, not copied;
# `index` int64 [rows], the table row t * N + n of every sample in the order the other entries are drawn; `cfg` the table's config. The ego of row r is
# entry 4 (agent_id) or 5 (share_agent_id) of the same tuple. gmpe.gnn_base_from_table consumes it: no [rows, E, F] and no [rows, E, E] batch is written.
TableRows = collections.namedtuple("TableRows", ("table", "index", "cfg"))
ADJ_MODES = ("matrix", "edges", "table")


def check_edge_args(adj, max_edge_dist, cap=None):
    """The arguments of an edge-list request, checked before anything is launched."""
    if adj not in ADJ_MODES:
        raise ValueError("adj must be one of %s (got %r)" % (ADJ_MODES, adj))
    if adj == "edges":
        if max_edge_dist is None or isinstance(max_edge_dist, bool) or not isinstance(max_edge_dist, numbers.Real) or max_edge_dist != max_edge_dist:
            raise ValueError('adj="edges" needs max_edge_dist (a number; the policy\'s args.max_edge_dist)')
    if cap is not None and (isinstance(cap, bool) or int(cap) != cap or int(cap) <= 0):
        raise ValueError("cap must be a positive integer or None (exact mode)")


def edge_list(cfg, device, source, src, T, N, A, E, max_edge_dist, perm=None, offset=0, rows=None, data_chunk_length=None, inclusive=False, index64=True,
              cap=None):
    """gmpe_minibatch_edges on one source: `source` _lib.MBE_ADJ / MBE_ADJ_COMPACT / MBE_TABLE, `src` the contiguous device tensor whose slot 0 is read
    ([T(+1), N, A, E, E] / [T(+1), N, E, E] f32 / [T(+1), N, W] f64). perm None: the identity. cap None: the exact mode — a count call, one read of the
    count, outputs of that size, a write call on the same workspace; cap int: one call, no host synchronisation. Enqueued on the current stream."""
    check_edge_args("edges", max_edge_dist, cap)
    lib = _lib.load()
    recurrent = data_chunk_length is not None
    L = int(data_chunk_length) if recurrent else 1
    rows = int(rows)
    graphs = rows * L
    if rows < 1:
        raise ValueError("rows must be >= 1")
    pl = _lib.GmpeMbEdgesPlan()
    pl.mode = _lib.MB_RECURRENT if recurrent else _lib.MB_FEED_FORWARD
    pl.source, pl.T, pl.N, pl.A, pl.L, pl.E = source, T, N, A, L, E
    pl.inclusive, pl.index64, pl.max_edge_dist = int(bool(inclusive)), int(bool(index64)), float(max_edge_dist)
    if perm is not None:
        pl.perm, pl.perm_len = perm.data_ptr(), int(perm.shape[0])
    pl.offset, pl.rows = int(offset), rows
    pl.src, pl.slot_stride = src.data_ptr(), src.stride(0) * src.element_size()
    nbytes = C.c_size_t()
    _lib.check(lib.gmpe_minibatch_edges_workspace_bytes(graphs, C.byref(nbytes)), "gmpe_minibatch_edges_workspace_bytes")
    ws = torch.empty((nbytes.value,), dtype=torch.uint8, device=device)
    ne = torch.empty((1,), dtype=torch.int32, device=device)
    pl.n_edges, pl.workspace, pl.workspace_bytes = ne.data_ptr(), ws.data_ptr(), nbytes.value
    idt = torch.int64 if index64 else torch.int32
    cfg_ref = C.byref(cfg) if cfg is not None else None
    stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    run = lambda: _lib.check(lib.gmpe_minibatch_edges(cfg_ref, device.index or 0, C.byref(pl), stream), "gmpe_minibatch_edges")
    if cap is None:
        run()                                                 # count only: edge_index is NULL
        m = int(ne.item())                                    # the one host synchronisation of the exact mode
        if m >= 2 ** 31 - 1:
            raise _lib.GmpeError("gmpe_minibatch_edges: more than 2^31 - 2 edges (the count saturates, include/gmpe.h): split the minibatch")
        ei = torch.empty((2, m), dtype=idt, device=device)
        ea = torch.empty((m, 1), dtype=torch.float32, device=device)
        if m:
            pl.edge_index, pl.edge_attr, pl.cap, pl.reuse_counts = ei.data_ptr(), ea.data_ptr(), m, 1
            run()
        return EdgeList(ei, ea, graphs, E, m)
    cap = int(cap)
    ei = torch.empty((2, cap), dtype=idt, device=device)
    ea = torch.empty((cap, 1), dtype=torch.float32, device=device)
    pl.edge_index, pl.edge_attr, pl.cap = ei.data_ptr(), ea.data_ptr(), cap
    run()
    return EdgeList(ei, ea, graphs, E, ne)


def table_index(units, T, N, A, data_chunk_length=None):
    """The table row t * N + n of every output row of a minibatch over `units` (int64 tensor: its slice of the permutation), in the gather's row order —
    sample_of's map (csrc/gmpe_mb_map.h) in torch's integer arithmetic, on the device `units` is on. Feed-forward (data_chunk_length None): unit u is
    sample u of the [T, N, A] order, so t * N + n = u // A. Recurrent: unit k is chunk c; its sample l is entry c * L + l of the [N, A, T] order and
    stands at output row l * len(units) + k."""
    if data_chunk_length is None:
        return units // A
    L = int(data_chunk_length)
    f = (units[None, :] * L + torch.arange(L, dtype=torch.int64, device=units.device)[:, None]).reshape(-1)
    return (f % T) * N + f // (A * T)


def _slot_array(name, t, lead, tail_dims, dtypes, device):
    """`t` must be a contiguous tensor [lead..., *tail] of one of `dtypes` on `device` (tail entries None: any size, at least 1), else ValueError."""
    shape_ok = isinstance(t, torch.Tensor) and t.dim() == len(lead) + len(tail_dims) and tuple(t.shape[:len(lead)]) == tuple(lead) and \
        all(d is None and s >= 1 or d == s for d, s in zip(tail_dims, t.shape[len(lead):]))
    if not shape_ok or t.dtype not in dtypes or not t.is_contiguous():
        want = tuple(lead) + tuple("*" if d is None else d for d in tail_dims)
        got = (tuple(t.shape), t.dtype) if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError("%s must be a contiguous %s tensor of shape %s (got %s)" % (name, "/".join(str(d) for d in dtypes), want, got))
    if t.device != device:
        raise ValueError("%s must be on %s (the device of the other arrays)" % (name, device))
    return t


class Gather(object):
    """The fields of one rollout's minibatches, checked and laid out once; calling it gathers one minibatch: perm[offset : offset + rows] (feed-forward: samples of the
    [T, N, A] flattening; recurrent: chunks of data_chunk_length samples in the [N, A, T] order) -> dict name -> fresh device tensor in the reference's batch shape.

    arrays: dict of device tensors, the buffer's names and shapes —
      obs f32 [T+1, N, A, D], agent_id i32 [T+1, N, A, 1], masks / active_masks f32 [T+1, N, A, 1]      (required)
      node_obs f32 [T+1, N, A, E, F] or entity_table f64 [T+1, N, W]                                   (one of them; rows win when both are given)
      adj f32 [T+1, N, A, E, E] or [T+1, N, E, E]; without it the matrices come from entity_table
      value_preds / returns f32 [T+1, N, A, 1], available_actions f32 [T+1, N, A, n_actions], advantages f32 [T, N, A, 1]
      rnn_states / rnn_states_critic [T+1, N, A, R, H], actions / action_log_probs [T, N, A, k]          (learner-owned; 4-byte dtypes, kept)
    Every name of TUPLE that cannot be formed is None in the result. share_obs / share_agent_id are obs[t, n] / agent_id[t, n] of all agents with
    use_centralized_V (DeviceRolloutBuffer.share_obs), the agent's own row without."""

    def __init__(self, cfg, arrays, data_chunk_length=None, use_centralized_V=True, adj="matrix"):
        check_edge_args(adj, 0.0)
        arrays = {k: v for k, v in dict(arrays).items() if v is not None}
        unknown = set(arrays) - set(TUPLE) - {"entity_table"}
        if unknown:
            raise ValueError("unknown arrays: %s" % sorted(unknown))
        for k in ("obs", "agent_id", "masks", "active_masks"):
            if k not in arrays:
                raise ValueError("arrays[%r] is required" % k)
        if adj == "edges" and "adj" not in arrays and "entity_table" not in arrays:
            raise ValueError('adj="edges" needs an adjacency form in the arrays: adj (materialised or compact) or the entity_table')
        if adj == "table" and "entity_table" not in arrays:
            raise ValueError('adj="table" needs the entity_table in the arrays (a buffer whose engine keeps tables: node_form "table" or "both")')
        obs = arrays["obs"]
        if not isinstance(obs, torch.Tensor) or obs.dim() != 4 or obs.shape[0] < 2:
            raise ValueError("obs must be a float32 tensor [T+1, N, A, D] with T >= 1")
        T1, N, A, D = (int(x) for x in obs.shape)
        T = T1 - 1
        if A != cfg.num_agents:
            raise ValueError("the arrays hold %d agents, the config %d" % (A, cfg.num_agents))
        dev = obs.device
        if dev.type != "cuda":
            raise ValueError("the arrays must be CUDA (HIP) device tensors: the minibatch gather has no CPU fallback")
        E, F, W, nact = cfg.num_entities, cfg.node_feats, cfg.entity_table_width, cfg.n_actions
        f32, i32 = (torch.float32,), (torch.int32,)
        full, half = (T1, N, A), (T, N, A)
        chk = lambda name, lead, tail, dt: _slot_array(name, arrays[name], lead, tail, dt, dev)
        self.recurrent = data_chunk_length is not None
        L = int(data_chunk_length) if self.recurrent else 1
        if L < 1:
            raise ValueError("data_chunk_length must be >= 1")
        self.cfg, self.device, self.T, self.N, self.A, self.L = cfg, dev, T, N, A, L
        fields = []                                          # (name, kind, tensor, slot bytes, row bytes, out dtype, row shape)

        def add(name, kind, t, row_bytes, dtype, row_shape):
            fields.append((name, kind, t, t.stride(0) * t.element_size(), int(row_bytes), dtype, tuple(row_shape)))

        chk("obs", full, (D,), f32)
        chk("agent_id", full, (1,), i32)
        if use_centralized_V:
            add("share_obs", _lib.MB_ENV_ROW, obs, A * D * 4, torch.float32, (A * D,))
        else:
            add("share_obs", _lib.MB_ROW, obs, D * 4, torch.float32, (D,))
        add("obs", _lib.MB_ROW, obs, D * 4, torch.float32, (D,))
        tab = arrays.get("entity_table")
        if tab is not None:
            chk("entity_table", (T1, N), (W,), (torch.float64,))
        self._table = tab
        nrows = len(fields)
        if "node_obs" in arrays:
            add("node_obs", _lib.MB_ROW, chk("node_obs", full, (E, F), f32), E * F * 4, torch.float32, (E, F))
        elif tab is not None:
            add("node_obs", _lib.MB_TABLE_NODE, tab, E * F * 4, torch.float32, (E, F))
        else:
            raise ValueError("arrays need node_obs rows or the entity_table")
        nfields = len(fields)
        if "adj" in arrays:
            a = arrays["adj"]
            if isinstance(a, torch.Tensor) and a.dim() == 4:
                add("adj", _lib.MB_ENV_ROW, chk("adj", (T1, N), (E, E), f32), E * E * 4, torch.float32, (E, E))
                self._edge_source = (_lib.MBE_ADJ_COMPACT, a)
            else:
                add("adj", _lib.MB_ROW, chk("adj", full, (E, E), f32), E * E * 4, torch.float32, (E, E))
                self._edge_source = (_lib.MBE_ADJ, a)
        elif tab is not None:
            add("adj", _lib.MB_TABLE_ADJ, tab, E * E * 4, torch.float32, (E, E))
            self._edge_source = (_lib.MBE_TABLE, tab)
        else:
            raise ValueError("arrays need an adjacency (adj) or the entity_table")
        self.adj_mode = adj
        if adj == "edges":
            del fields[nfields:]                             # no [rows, E, E] batch: the minibatch's entry 3 is the EdgeList (edges)
        elif adj == "table":
            del fields[nrows:]                               # ... nor a [rows, E, F] one: entry 2 is None, entry 3 the TableRows (table_rows)
        ids = arrays["agent_id"]
        add("agent_id", _lib.MB_ROW, ids, 4, torch.int32, (1,))
        if use_centralized_V:
            add("share_agent_id", _lib.MB_ENV_ROW, ids, A * 4, torch.int32, (A,))
        else:
            add("share_agent_id", _lib.MB_ROW, ids, 4, torch.int32, (1,))
        for name in ("rnn_states", "rnn_states_critic"):
            if name in arrays:
                t = _slot_array(name, arrays[name], full, (None, None), (torch.float32, torch.int32), dev)
                add(name, _lib.MB_CHUNK_HEAD if self.recurrent else _lib.MB_ROW, t, t[0, 0, 0].numel() * 4, t.dtype, tuple(t.shape[3:]))
        for name in ("actions",):
            if name in arrays:
                t = _slot_array(name, arrays[name], half, (None,), (torch.float32, torch.int32), dev)
                add(name, _lib.MB_ROW, t, t.shape[3] * 4, t.dtype, (t.shape[3],))
        for name in ("value_preds", "returns", "masks", "active_masks"):
            if name in arrays:
                add(name, _lib.MB_ROW, chk(name, full, (1,), f32), 4, torch.float32, (1,))
        if "action_log_probs" in arrays:
            t = _slot_array("action_log_probs", arrays["action_log_probs"], half, (None,), (torch.float32, torch.int32), dev)
            add("action_log_probs", _lib.MB_ROW, t, t.shape[3] * 4, t.dtype, (t.shape[3],))
        if "advantages" in arrays:
            add("advantages", _lib.MB_ROW, chk("advantages", half, (1,), f32), 4, torch.float32, (1,))
        if "available_actions" in arrays:
            add("available_actions", _lib.MB_ROW, chk("available_actions", full, (nact,), f32), nact * 4, torch.float32, (nact,))
        self.fields = fields
        self.names = [f[0] for f in fields]
        self._keep = arrays                                  # the sources stay alive while the plan points at them
        plan = _lib.GmpeMinibatchPlan()
        plan.mode = _lib.MB_RECURRENT if self.recurrent else _lib.MB_FEED_FORWARD
        plan.num_fields = len(fields)
        plan.T, plan.N, plan.A, plan.L = T, N, A, L
        for i, (name, kind, t, slot, row, _, _) in enumerate(fields):
            f = plan.fields[i]
            f.kind, f.row_bytes, f.slot_stride, f.src = kind, row, slot, t.data_ptr()
        self.plan = plan
        self._cfg_ref = C.byref(cfg)
        self._lib = _lib.load()

    @property
    def num_units(self):
        """samples (feed-forward) or chunks (recurrent) a permutation ranges over"""
        n = self.T * self.N * self.A
        return n // self.L if self.recurrent else n

    def out_bytes(self, rows):
        """bytes one minibatch of `rows` samples / chunks writes"""
        return sum(self._rows(kind, rows) * row for _, kind, _, _, row, _, _ in self.fields)

    def _rows(self, kind, rows):
        return rows * self.L if self.recurrent and kind != _lib.MB_CHUNK_HEAD else rows

    def __call__(self, perm, offset, rows):
        """perm: int64 device tensor; the minibatch perm[offset : offset + rows]. Returns dict name -> fresh tensor (one slab), enqueued on the current stream."""
        if not isinstance(perm, torch.Tensor) or perm.dtype != torch.int64 or perm.dim() != 1 or not perm.is_contiguous() or perm.device != self.device:
            raise ValueError("perm must be a contiguous 1-D int64 tensor on %s" % self.device)
        offset, rows = int(offset), int(rows)
        if rows < 1 or offset < 0 or offset + rows > perm.shape[0]:
            raise ValueError("the minibatch [%d, %d) does not lie in the permutation's %d entries" % (offset, offset + rows, perm.shape[0]))
        offs, total = [], 0
        for _, kind, _, _, row, _, _ in self.fields:
            offs.append(total)
            total += -(-self._rows(kind, rows) * row // _ALIGN) * _ALIGN
        slab = torch.empty((total,), dtype=torch.uint8, device=self.device)
        base = slab.data_ptr()
        p = self.plan
        p.perm, p.perm_len, p.offset, p.rows = perm.data_ptr(), int(perm.shape[0]), offset, rows
        out = {}
        for i, ((name, kind, _, _, row, dt, shape), o) in enumerate(zip(self.fields, offs)):
            n = self._rows(kind, rows)
            p.fields[i].dst = base + o
            out[name] = slab[o:o + n * row].view(dt).view((n,) + shape)
        _lib.check(self._lib.gmpe_minibatch_gather(self._cfg_ref, self.device.index or 0, C.byref(p),
                                                   C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)), "gmpe_minibatch_gather")
        return out

    def edges(self, perm, offset, rows, max_edge_dist, inclusive=False, index64=True, cap=None):
        """The edge list of the minibatch perm[offset : offset + rows] (perm None: the identity) — process_adj of the adj batch __call__ would return, graph r its
        row r — straight from the stored adjacency form: -> EdgeList. cap None: exact sizes, one host synchronisation; cap int: [2, cap] / [cap, 1] outputs,
        n_edges a device tensor, no synchronisation (truncation is the caller's to check)."""
        check_edge_args("edges", max_edge_dist, cap)
        if perm is not None and (not isinstance(perm, torch.Tensor) or perm.dtype != torch.int64 or perm.dim() != 1 or not perm.is_contiguous()
                                 or perm.device != self.device):
            raise ValueError("perm must be None or a contiguous 1-D int64 tensor on %s" % self.device)
        offset, rows = int(offset), int(rows)
        n = self.num_units if perm is None else perm.shape[0]
        if rows < 1 or offset < 0 or offset + rows > n:
            raise ValueError("the minibatch [%d, %d) does not lie in the permutation's %d entries" % (offset, offset + rows, n))
        source, src = self._edge_source
        return edge_list(self.cfg, self.device, source, src, self.T, self.N, self.A, self.cfg.num_entities, max_edge_dist, perm=perm, offset=offset, rows=rows,
                         data_chunk_length=self.L if self.recurrent else None, inclusive=inclusive, index64=index64, cap=cap)

    def table_rows(self, perm, offset, rows):
        """The TableRows of the minibatch perm[offset : offset + rows]: the buffer's own entity table and, per output row of __call__, its table row
        t * N + n — sample_of's map (csrc/gmpe_mb_map.h) in torch's integer arithmetic on the device. Enqueued on the current stream; nothing is gathered."""
        if self._table is None:
            raise ValueError('table_rows needs the entity_table in the arrays (a buffer whose engine keeps tables: node_form "table" or "both")')
        units = perm[int(offset):int(offset) + int(rows)]
        return TableRows(self._table, table_index(units, self.T, self.N, self.A, self.L if self.recurrent else None), self.cfg)

    def tuple(self, out):
        """the reference's 16-tuple order (None where a field was not given)"""
        return tuple(out.get(k) for k in TUPLE)


def minibatch(cfg, arrays, perm, offset, rows, data_chunk_length=None, use_centralized_V=True):
    """One minibatch: Gather(cfg, arrays, data_chunk_length, use_centralized_V)(perm, offset, rows). Build a Gather once to draw several."""
    return Gather(cfg, arrays, data_chunk_length, use_centralized_V)(perm, offset, rows)


# ---------------------------------------------------------------------- the reference's samplers
def feed_forward_sizes(T, N, A, num_mini_batch=None, mini_batch_size=None):
    """graph_buffer.py:385-399: (batch_size, mini_batch_size, [(offset, rows) per minibatch]) — slices of the permutation, remainders never sampled."""
    batch = N * T * A
    if mini_batch_size is None:
        assert batch >= num_mini_batch, (
            f"PPO requires the number of processes ({N}) "
            f"* number of steps ({T}) * number of agents "
            f"({A}) = {N * T * A} "
            "to be greater than or equal to the number of "
            f"PPO mini batches ({num_mini_batch}).")
        mini_batch_size = batch // num_mini_batch
    if num_mini_batch is None:
        raise ValueError("num_mini_batch is required (the reference iterates range(num_mini_batch))")
    mbs = int(mini_batch_size)
    return batch, mbs, [(i * mbs, max(0, min(batch, (i + 1) * mbs) - i * mbs)) for i in range(int(num_mini_batch))]


def recurrent_sizes(T, N, A, num_mini_batch, data_chunk_length):
    """graph_buffer.py:617-622: (data_chunks, chunks per minibatch, [(offset, chunks) per minibatch])."""
    batch = N * T * A
    data_chunks = batch // int(data_chunk_length)
    mbc = data_chunks // int(num_mini_batch)
    return data_chunks, mbc, [(i * mbc, max(0, min(data_chunks, (i + 1) * mbc) - i * mbc)) for i in range(int(num_mini_batch))]


def device_perm(perm, n, device):
    """The permutation of a generator call as an int64 device tensor: None -> torch.randperm(n) on the CPU default generator (the reference's draw), uploaded once
    (pinned, non-blocking); "device" -> drawn on the device (no host work, other draws); a tensor -> checked once for shape, dtype and range."""
    if perm is None:
        cpu = torch.randperm(n)
        return cpu.pin_memory().to(device, non_blocking=True)
    if isinstance(perm, str):
        if perm != "device":
            raise ValueError('perm must be None, "device" or an int64 tensor')
        return torch.randperm(n, device=device)
    if not isinstance(perm, torch.Tensor) or perm.dtype != torch.int64 or tuple(perm.shape) != (n,):
        raise ValueError("perm must be an int64 tensor of shape (%d,)" % n)
    if n and (int(perm.min()) < 0 or int(perm.max()) >= n):
        raise ValueError("perm entries must lie in [0, %d)" % n)
    return perm.to(device).contiguous()


def _empty(g):
    """what the reference yields for a slice of the permutation that is empty (mini_batch_size beyond the batch): zero-row arrays"""
    return {name: torch.empty((0,) + shape, dtype=dt, device=g.device) for name, _, _, _, _, dt, shape in g.fields}


def feed_forward_generator(cfg, arrays, advantages, num_mini_batch=None, mini_batch_size=None, perm=None, use_centralized_V=True, adj="matrix",
                           max_edge_dist=None, inclusive=False):
    """GraphReplayBuffer.feed_forward_generator on the device: yields the reference's 16-tuple per minibatch (available_actions_batch None without
    available_actions). The arguments are checked here; the permutation is drawn at the first next(), as the reference's.
    adj="edges": entry 3 of the tuple is the minibatch's EdgeList (process_adj with max_edge_dist; exact sizes) and no adj batch is written.
    adj="table" (the arrays must hold the entity_table): entry 2 is None and entry 3 the minibatch's TableRows — the table itself and one int64 per row —,
    so neither the node rows nor the matrices are written; gmpe.policy's layers run gnn_base_from_table on it."""
    check_edge_args(adj, max_edge_dist)
    if advantages is None:
        raise ValueError("feed_forward_generator needs the advantages (the reference reshapes them unconditionally, graph_buffer.py:422)")
    arrays = dict(arrays, advantages=advantages)
    g = Gather(cfg, arrays, None, use_centralized_V, adj=adj)
    _, _, sampler = feed_forward_sizes(g.T, g.N, g.A, num_mini_batch, mini_batch_size)
    return _run(g, sampler, perm, max_edge_dist, inclusive)


def recurrent_generator(cfg, arrays, advantages, num_mini_batch, data_chunk_length, perm=None, use_centralized_V=True, adj="matrix", max_edge_dist=None,
                        inclusive=False):
    """GraphReplayBuffer.recurrent_generator on the device: chunks of data_chunk_length samples in the [N, A, T] order (a chunk crosses agent / env boundaries
    when T % L != 0, as the reference's), rows l * chunks + k, rnn states from each chunk's first sample. adj="edges": as feed_forward_generator."""
    check_edge_args(adj, max_edge_dist)
    if advantages is None:
        raise ValueError("recurrent_generator needs the advantages (the reference casts them unconditionally, graph_buffer.py:632)")
    arrays = dict(arrays, advantages=advantages)
    g = Gather(cfg, arrays, int(data_chunk_length), use_centralized_V, adj=adj)
    data_chunks, mbc, sampler = recurrent_sizes(g.T, g.N, g.A, num_mini_batch, data_chunk_length)
    if mbc < 1:
        raise ValueError("recurrent_generator: %d chunks of %d samples do not fill %d minibatches (the reference's np.stack of an empty list fails)"
                         % (data_chunks, int(data_chunk_length), int(num_mini_batch)))
    return _run(g, sampler, perm, max_edge_dist, inclusive)


def _empty_edges(g):
    return EdgeList(torch.empty((2, 0), dtype=torch.int64, device=g.device), torch.empty((0, 1), dtype=torch.float32, device=g.device), 0,
                    g.cfg.num_entities, 0)


def _run(g, sampler, perm, max_edge_dist=None, inclusive=False):
    n = g.num_units
    if perm is not None and not isinstance(perm, str):
        perm = device_perm(perm, n, g.device)                # checked once, before the first next()
    elif isinstance(perm, str) and perm != "device":
        raise ValueError('perm must be None, "device" or an int64 tensor')

    def gen(perm=perm):
        p = device_perm(perm, n, g.device) if perm is None or isinstance(perm, str) else perm
        for off, rows in sampler:
            out = g(p, off, rows) if rows else _empty(g)
            if g.adj_mode == "edges":
                out["adj"] = g.edges(p, off, rows, max_edge_dist, inclusive) if rows else _empty_edges(g)
            elif g.adj_mode == "table":
                out["adj"] = g.table_rows(p, off, rows)
            yield g.tuple(out)
    return gen()
