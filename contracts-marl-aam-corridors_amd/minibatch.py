"""PPO minibatches drawn on the device from a rollout's [T+1, N, ...] arrays (GraphReplayBuffer.feed_forward_generator / recurrent_generator,
onpolicy/utils/graph_buffer.py:368-758, called by GR_MAPPO.train, onpolicy/algorithms/graph_mappo.py:319-331).

One minibatch is one gmpe_minibatch_gather call (include/gmpe.h; csrc/gmpe_minibatch.hip): every field's rows are gathered through the device permutation into one
fresh slab, in the reference's shapes, dtypes and order — the 16-tuple ppo_update consumes unchanged. The arrays may be in any storage form of the rollout buffer:
node rows or the fp64 entity table, materialised [.., A, E, E] / compact [.., E, E] / no adjacency (rebuilt from the table, bit-identical to the engine). No engine
is needed, so a learner rank can run this on a ShardedRolloutCollector.unpack result or on raw entity tables.
"""
import ctypes as C

import torch

from . import _lib

# the reference's yield order (graph_buffer.py:461-465, 753-757); "advantages" is adv_targ, "action_log_probs" old_action_log_probs_batch
TUPLE = ("share_obs", "obs", "node_obs", "adj", "agent_id", "share_agent_id", "rnn_states", "rnn_states_critic", "actions", "value_preds", "returns", "masks",
         "active_masks", "action_log_probs", "advantages", "available_actions")
LEARNER = ("rnn_states", "rnn_states_critic", "actions", "action_log_probs")
_ALIGN = 256


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

    def __init__(self, cfg, arrays, data_chunk_length=None, use_centralized_V=True):
        arrays = {k: v for k, v in dict(arrays).items() if v is not None}
        unknown = set(arrays) - set(TUPLE) - {"entity_table"}
        if unknown:
            raise ValueError("unknown arrays: %s" % sorted(unknown))
        for k in ("obs", "agent_id", "masks", "active_masks"):
            if k not in arrays:
                raise ValueError("arrays[%r] is required" % k)
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
        if "node_obs" in arrays:
            add("node_obs", _lib.MB_ROW, chk("node_obs", full, (E, F), f32), E * F * 4, torch.float32, (E, F))
        elif tab is not None:
            add("node_obs", _lib.MB_TABLE_NODE, tab, E * F * 4, torch.float32, (E, F))
        else:
            raise ValueError("arrays need node_obs rows or the entity_table")
        if "adj" in arrays:
            a = arrays["adj"]
            if isinstance(a, torch.Tensor) and a.dim() == 4:
                add("adj", _lib.MB_ENV_ROW, chk("adj", (T1, N), (E, E), f32), E * E * 4, torch.float32, (E, E))
            else:
                add("adj", _lib.MB_ROW, chk("adj", full, (E, E), f32), E * E * 4, torch.float32, (E, E))
        elif tab is not None:
            add("adj", _lib.MB_TABLE_ADJ, tab, E * E * 4, torch.float32, (E, E))
        else:
            raise ValueError("arrays need an adjacency (adj) or the entity_table")
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


def feed_forward_generator(cfg, arrays, advantages, num_mini_batch=None, mini_batch_size=None, perm=None, use_centralized_V=True):
    """GraphReplayBuffer.feed_forward_generator on the device: yields the reference's 16-tuple per minibatch (available_actions_batch None without
    available_actions). The arguments are checked here; the permutation is drawn at the first next(), as the reference's."""
    if advantages is None:
        raise ValueError("feed_forward_generator needs the advantages (the reference reshapes them unconditionally, graph_buffer.py:422)")
    arrays = dict(arrays, advantages=advantages)
    g = Gather(cfg, arrays, None, use_centralized_V)
    _, _, sampler = feed_forward_sizes(g.T, g.N, g.A, num_mini_batch, mini_batch_size)
    return _run(g, sampler, perm)


def recurrent_generator(cfg, arrays, advantages, num_mini_batch, data_chunk_length, perm=None, use_centralized_V=True):
    """GraphReplayBuffer.recurrent_generator on the device: chunks of data_chunk_length samples in the [N, A, T] order (a chunk crosses agent / env boundaries
    when T % L != 0, as the reference's), rows l * chunks + k, rnn states from each chunk's first sample."""
    if advantages is None:
        raise ValueError("recurrent_generator needs the advantages (the reference casts them unconditionally, graph_buffer.py:632)")
    arrays = dict(arrays, advantages=advantages)
    g = Gather(cfg, arrays, int(data_chunk_length), use_centralized_V)
    data_chunks, mbc, sampler = recurrent_sizes(g.T, g.N, g.A, num_mini_batch, data_chunk_length)
    if mbc < 1:
        raise ValueError("recurrent_generator: %d chunks of %d samples do not fill %d minibatches (the reference's np.stack of an empty list fails)"
                         % (data_chunks, int(data_chunk_length), int(num_mini_batch)))
    return _run(g, sampler, perm)


def _run(g, sampler, perm):
    n = g.num_units
    if perm is not None and not isinstance(perm, str):
        perm = device_perm(perm, n, g.device)                # checked once, before the first next()
    elif isinstance(perm, str) and perm != "device":
        raise ValueError('perm must be None, "device" or an int64 tensor')

    def gen(perm=perm):
        p = device_perm(perm, n, g.device) if perm is None or isinstance(perm, str) else perm
        for off, rows in sampler:
            yield g.tuple(g(p, off, rows) if rows else _empty(g))
    return gen()
