"""GmpeEngine — thin Python owner of one gmpe_handle (one per GPU) + the torch output buffers.

PyTorch is plumbing only: device memory (`torch.empty(..., device=...)`), streams and
`torch.distributed`. All arithmetic happens in the HIP kernels behind include/gmpe.h.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .config import FIELDS, INFO_KEYS, NODE_FEATS, GmpeConfig, algorithmic_bytes_per_env_step


class StepOutputs(object):
    """Device-resident outputs of one step/reset (torch tensors on the engine's device)."""
    __slots__ = ("obs", "agent_id", "node_obs", "adj", "reward", "done", "info", "entity_table")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


class GmpeEngine(object):
    def __init__(self, cfg, device=0, adj_compact=False, with_info=True, node_form="rows", adj_form=None):
        """node_form: "rows" — the engine writes node_obs [N,A,E,F] (what GraphSubprocVecEnv hands the runner); "table" — it writes the fp64 entity table
        [N,W] instead (include/gmpe.h gmpe_outputs.entity_table: the state the rows are a pure function of, ~8x fewer bytes — the form a rank ships to the learner,
        expanded there by expand_node_obs); "both" — both outputs.
        adj_form: None — by `adj_compact` ([N,E,E] or [N,A,E,E]); "none" — no adjacency output at all: the matrix is a function of the entity table too (positions +
        mask words, expand_adj), so a rank that ships the table need not write or ship it (needs node_form "table" or "both")."""
        if not isinstance(cfg, GmpeConfig):
            raise TypeError("cfg must be a gmpe.config.GmpeConfig")
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.GmpeError("no MI355X visible to torch: the engine has no CPU fallback")
        self.cfg = cfg
        self.device = torch.device("cuda", int(device))
        self.N, self.A = cfg.num_envs, cfg.num_agents
        self.E, self.D = cfg.num_entities, cfg.obs_dim
        self.adj_compact = bool(adj_compact)
        if node_form not in ("rows", "table", "both"):
            raise ValueError("node_form must be 'rows', 'table' or 'both'")
        self.node_form = node_form
        if adj_form not in (None, "none"):
            raise ValueError("adj_form must be None (by adj_compact) or 'none'")
        if adj_form == "none" and node_form == "rows":
            raise ValueError("adj_form='none' needs the entity table (node_form 'table' or 'both'): the adjacency is rebuilt from it")
        self.adj_form = "none" if adj_form == "none" else ("compact" if adj_compact else "full")
        self.h = C.c_void_p()
        _lib.check(self.lib.gmpe_create(C.byref(cfg), self.device.index, C.byref(self.h)), "gmpe_create")
        N, A, E, D = self.N, self.A, self.E, self.D
        dev = self.device
        self.out = StepOutputs(
            obs=torch.empty((N, A, D), dtype=torch.float32, device=dev),
            agent_id=torch.empty((N, A, 1), dtype=torch.int32, device=dev),
            node_obs=torch.empty((N, A, E, cfg.node_feats), dtype=torch.float32, device=dev) if node_form != "table" else None,
            entity_table=torch.empty((N, cfg.entity_table_width), dtype=torch.float64, device=dev) if node_form != "rows" else None,
            adj=None if adj_form == "none" else torch.empty((N, E, E) if adj_compact else (N, A, E, E), dtype=torch.float32, device=dev),
            reward=torch.empty((N, A), dtype=torch.float32, device=dev),
            done=torch.empty((N, A), dtype=torch.uint8, device=dev),
            info=torch.empty((N, A, len(INFO_KEYS)), dtype=torch.float32, device=dev) if with_info else None)
        self._tape = None
        self._ovr = None
        self._timing = False
        self._o = self._pack(self.out)

    # ------------------------------------------------------------------ plumbing
    def _pack(self, o):
        p = lambda t: None if t is None else t.data_ptr()
        return _lib.GmpeOutputs(p(o.obs), p(o.agent_id), p(o.node_obs), p(o.adj), p(o.reward), p(o.done),
                                p(o.info), int(self.adj_compact), 0, p(o.entity_table))

    def rebind(self, outputs):
        """Point the engine at other caller-owned output tensors (same shapes/dtypes, same device)."""
        self._check_outputs(outputs)
        self.out = outputs
        self._o = self._pack(outputs)

    def _check_outputs(self, o, partial=False, num_slots=1, strides=None):
        """`o` against the engine's own outputs: same shape and dtype, on this device, contiguous. Presence must match, except that with partial=True an absent
        output is allowed (it is not written). With num_slots > 1 the storage behind every output must also hold num_slots slots at its entry in `strides`."""
        for k in StepOutputs.__slots__:
            a, b = getattr(self.out, k), getattr(o, k)
            if b is None and (a is None or partial):
                continue
            if a is None or b is None:
                raise ValueError("output %r: presence differs" % k)
            if tuple(a.shape) != tuple(b.shape) or a.dtype != b.dtype or b.device != self.device or not b.is_contiguous():
                raise ValueError("output %r must be a contiguous %s tensor of shape %s on %s" % (k, a.dtype, tuple(a.shape), self.device))
            if num_slots > 1:
                _check_slots(k, b, b.numel(), num_slots, int((strides or {}).get(k, 0)))

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def close(self):
        if getattr(self, "h", None):
            self.lib.gmpe_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ hot path
    def reset(self, mask=None):
        m = None
        if mask is not None:
            m = torch.as_tensor(mask, dtype=torch.uint8, device=self.device).contiguous()
        _lib.check(self.lib.gmpe_reset(self.h, None if m is None else m.data_ptr(), C.byref(self._o),
                                       self._stream()), "gmpe_reset")
        return self.out

    def _actions(self, a, dtype, numel, convert, msg):
        """`a` as a contiguous `dtype` tensor on this device with `numel` elements: converted when `convert`, refused (ValueError `msg`) otherwise."""
        if a.dtype != dtype or not a.is_contiguous() or a.device != self.device:
            a = a.to(device=self.device, dtype=dtype).contiguous() if convert else None
        if a is None or a.numel() != numel:
            raise ValueError(msg)
        return a

    def step(self, action_idx):
        """action_idx: int32 device tensor [N,A]."""
        a = self._actions(action_idx, torch.int32, self.N * self.A, True, "action_idx must have N*A = %d elements" % (self.N * self.A))
        _lib.check(self.lib.gmpe_step(self.h, a.data_ptr(), C.byref(self._o), self._stream()), "gmpe_step")
        return self.out

    def step_envs(self, action_idx, env_lo, env_hi, stream=None):
        """Step the envs [env_lo, env_hi) only (whole-batch `action_idx` [N,A] and outputs; rows outside the range untouched), on `stream`
        (a torch.cuda.Stream; default: the current one). Ranges are independent: a runner can double-buffer halves of the batch."""
        a = self._actions(action_idx, torch.int32, self.N * self.A, False,
                          "action_idx must be a contiguous int32 device tensor with N*A = %d elements" % (self.N * self.A))
        st = C.c_void_p(stream.cuda_stream) if stream is not None else self._stream()
        _lib.check(self.lib.gmpe_step_envs(self.h, a.data_ptr(), C.byref(self._o), int(env_lo), int(env_hi), st), "gmpe_step_envs")
        return self.out

    def step_many_ranges(self, action_sets, num_steps, parts=2):
        """num_steps open-loop steps with the batch cut into `parts` env ranges, each on its own side stream (gmpe_step_many_envs)."""
        a = action_sets
        self._check_action_sets(a)
        _lib.check(self.lib.gmpe_step_many_envs(self.h, a.data_ptr(), int(num_steps), int(a.shape[0]), C.byref(self._o), int(parts), self._stream()),
                   "gmpe_step_many_envs")
        return self.out

    def _check_action_sets(self, a):
        if a.dtype != torch.int32 or not a.is_contiguous() or a.device != self.device or a.dim() != 3:
            raise ValueError("action_sets must be a contiguous int32 device tensor [S, N, A]")
        if a.shape[1] * a.shape[2] != self.N * self.A:
            raise ValueError("action_sets must be [S, %d, %d]" % (self.N, self.A))

    def step_many_prepare(self, action_sets, num_steps):
        """Record the launches of step_many(action_sets, num_steps) into a hipGraph (once, off the step path); later
        step_many calls with the same tensor / count / outputs replay it with one graph launch."""
        self._check_action_sets(action_sets)
        _lib.check(self.lib.gmpe_step_many_prepare(self.h, action_sets.data_ptr(), int(num_steps), int(action_sets.shape[0]),
                                                   C.byref(self._o)), "gmpe_step_many_prepare")

    def step_many(self, action_sets, num_steps):
        """Open-loop rollout: `num_steps` steps enqueued by one C call — one launch of the persistent rollout kernel unless the
        handle's tuning says otherwise; step k uses action_sets[k % len] (int32 device tensor [S, N, A]). Returns the outputs of
        the LAST step."""
        a = action_sets
        self._check_action_sets(a)
        _lib.check(self.lib.gmpe_step_many(self.h, a.data_ptr(), int(num_steps), int(a.shape[0]), C.byref(self._o),
                                           self._stream()), "gmpe_step_many")
        return self.out

    def rollout(self, action_sets, num_steps, slot0=None, num_slots=1, first_slot=0, strides=None, masks=None, active_masks=None):
        """K steps in ONE launch (gmpe_rollout_steps, the persistent rollout kernel). Step k reads action_sets[k % S] and writes
        output slot (first_slot + k) % num_slots: `slot0` = StepOutputs of slot 0 (default: the engine's own buffers),
        `strides` = dict output-name -> elements between consecutive slots (default 0). Bit-identical to `num_steps` step() calls."""
        self.prepare_rollout(action_sets, num_steps, slot0, num_slots, first_slot, strides, masks, active_masks)()
        return self.out

    def prepare_rollout(self, action_sets, num_steps, slot0=None, num_slots=1, first_slot=0, strides=None, masks=None, active_masks=None):
        """The launch of rollout(...) with these arguments as a callable: the argument structs (gmpe_rollout, gmpe_outputs) are built once, a call is ONE C call
        (gmpe_rollout_steps on the current stream). For collect loops that launch the same rollout every episode — building slot views and structs in Python costs
        ~30 us per launch, 7 % of a 20-step rollout at c2. The tensors are referenced, not copied: their contents are read / written at launch time.
        Every argument is checked here, before anything is launched: `slot0` like rebind's outputs (an absent output is not written), and the storage behind every
        output and mask must hold `num_slots` slots at its stride. With slot0=None the callable writes the outputs the engine is bound to NOW and keeps them alive:
        a later rebind points the engine elsewhere but does not free them under it."""
        a = action_sets
        self._check_action_sets(a)
        st = strides or {}
        outs = self.out if slot0 is None else slot0
        self._check_outputs(outs, partial=True, num_slots=int(num_slots), strides=st)
        for k, m in (("masks", masks), ("active_masks", active_masks)):
            if m is not None:
                if m.dtype != torch.float32 or m.device != self.device or not m.is_contiguous():
                    raise ValueError("%s must be a contiguous float32 tensor on %s" % (k, self.device))
                _check_slots(k, m, self.N * self.A, int(num_slots), int(st.get("masks", 0)))
        o = self._pack(outs)
        r = _lib.GmpeRollout(int(num_steps), int(a.shape[0]), int(num_slots), int(first_slot),
                             int(st.get("obs", 0)), int(st.get("agent_id", 0)), int(st.get("node_obs", 0)), int(st.get("adj", 0)),
                             int(st.get("reward", 0)), int(st.get("done", 0)), int(st.get("info", 0)), int(st.get("masks", 0)),
                             None if masks is None else masks.data_ptr(), None if active_masks is None else active_masks.data_ptr(),
                             int(st.get("entity_table", 0)))
        keep = (a, masks, active_masks) + tuple(getattr(outs, k) for k in StepOutputs.__slots__)   # the tensors behind the raw pointers stay alive with the callable
        eng, fn, ap, rp, op, stream, check = self, self.lib.gmpe_rollout_steps, a.data_ptr(), C.byref(r), C.byref(o), self._stream, _lib.check

        def launch(_keep=keep, _r=r, _o=o):
            h = eng.h                                                    # read at launch time: a closed engine must fail loudly, not hand the C side a freed handle
            if not h:
                raise _lib.GmpeError("prepared rollout launched after the engine was closed")
            check(fn(h, ap, rp, op, stream()), "gmpe_rollout_steps")
        return launch

    def tuning(self):
        """What gmpe_create chose (tile shape, store flavour, split / rollout paths) as a dict."""
        t = _lib.GmpeTuning()
        _lib.check(self.lib.gmpe_get_tuning(self.h, C.byref(t)), "gmpe_get_tuning")
        return {k: int(getattr(t, k)) for k, _ in _lib.GmpeTuning._fields_ if k != "reserved"}

    def step_many_loop(self, action_sets, num_steps):
        """step_many as one kernel launch per step (the closed-loop launch shape; replays a prepared hipGraph when there is one)."""
        a = action_sets
        self._check_action_sets(a)
        _lib.check(self.lib.gmpe_step_many_launches(self.h, a.data_ptr(), int(num_steps), int(a.shape[0]), C.byref(self._o),
                                                    self._stream()), "gmpe_step_many_launches")
        return self.out

    def step_onehot(self, onehot):
        """onehot: float32 device tensor [N,A,n_actions] (argmax fused into the kernel)."""
        a = self._actions(onehot, torch.float32, self.N * self.A * self.cfg.n_actions, True, "onehot must be [N,A,%d]" % self.cfg.n_actions)
        _lib.check(self.lib.gmpe_step_onehot(self.h, a.data_ptr(), C.byref(self._o), self._stream()),
                   "gmpe_step_onehot")
        return self.out

    # ------------------------------------------------------------------ state access
    def get(self, name):
        fid, dt, shp = FIELDS[name]
        a = np.empty(shp(self.cfg), dtype=dt)
        _lib.check(self.lib.gmpe_get_field(self.h, fid, a.ctypes.data_as(C.c_void_p), a.nbytes), "gmpe_get_field")
        return a

    def set(self, name, value):
        fid, dt, shp = FIELDS[name]
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(value, dtype=dt), shp(self.cfg)))
        _lib.check(self.lib.gmpe_set_field(self.h, fid, a.ctypes.data_as(C.c_void_p), a.nbytes), "gmpe_set_field")

    def get_state(self):
        return {k: self.get(k) for k in FIELDS}

    def set_state(self, state):
        for k, v in state.items():
            self.set(k, v)

    def set_tape(self, tape):
        """Parity mode: f64 [N, len] of [0,1) samples replayed instead of Philox (None to disable)."""
        if tape is None:
            self._tape = None
            _lib.check(self.lib.gmpe_set_rng_tape(self.h, None, 0), "gmpe_set_rng_tape")
            return
        t = torch.as_tensor(np.asarray(tape, dtype=np.float64).reshape(self.N, -1), device=self.device).contiguous()
        torch.cuda.synchronize(self.device)
        self._tape = t
        _lib.check(self.lib.gmpe_set_rng_tape(self.h, t.data_ptr(), t.shape[1]), "gmpe_set_rng_tape")

    def set_control_override(self, ctrl=None, use=None):
        """Safety-filter hook slot (multiagent/core.py:692-736): `ctrl` float64 device tensor [N,A,2] integrated instead of the decoded
        action wherever `use` (uint8 [N,A]; None = everywhere) is non-zero. None removes the hook. The tensors are read at step time
        (the engine keeps references)."""
        if ctrl is None:
            self._ovr = None
            _lib.check(self.lib.gmpe_set_control_override(self.h, None, None), "gmpe_set_control_override")
            return
        if ctrl.dtype != torch.float64 or tuple(ctrl.shape) != (self.N, self.A, 2) or not ctrl.is_contiguous() or ctrl.device != self.device:
            raise ValueError("ctrl must be a contiguous float64 device tensor [N, A, 2]")
        if use is not None and (use.dtype != torch.uint8 or use.numel() != self.N * self.A or not use.is_contiguous() or use.device != self.device):
            raise ValueError("use must be a contiguous uint8 device tensor [N, A]")
        self._ovr = (ctrl, use)
        _lib.check(self.lib.gmpe_set_control_override(self.h, ctrl.data_ptr(), None if use is None else use.data_ptr()), "gmpe_set_control_override")

    def state_tensor(self, name):
        """Zero-copy torch view of a state field in HBM (gmpe_field_device_ptr), e.g. for an on-device safety filter that reads
        x / y / s2 / s3 before the step. Same stream as the engine's launches; do not resize or free."""
        fid, dt, shp = FIELDS[name]
        p = C.c_void_p()
        _lib.check(self.lib.gmpe_field_device_ptr(self.h, fid, C.byref(p)), "gmpe_field_device_ptr")
        shape = tuple(int(x) for x in shp(self.cfg))

        class _Blob(object):
            __cuda_array_interface__ = {"shape": shape, "typestr": np.dtype(dt).str, "data": (int(p.value), False), "version": 2, "strides": None}
        return torch.as_tensor(_Blob(), device=self.device)

    def check_errors(self):
        e = self.get("error_flags")
        if (e & 1).any():
            raise _lib.GmpeError("RNG tape exhausted in %d env(s)" % int((e & 1).astype(bool).sum()))
        if (e & 2).any():
            raise _lib.GmpeError("reset placement gave up in %d env(s) (world too small for the agents)"
                                 % int((e & 2).astype(bool).sum()))

    # ------------------------------------------------------------------ edges (learner-side process_adj)
    def edges_from_adj(self, adj, max_edge_dist, inclusive=False, cap=None, index64=False):
        """process_adj's edge set (gnn_new.py:329-358) of a materialised [B, E, E] (or [N, A, E, E]) adjacency: -> (edge_index [2, M] int32 — int64
        with index64=True, what torch.nonzero / PyG message passing use —, edge_attr [M], M). Prefer edges_from_adj_compact when the
        engine writes the compact adjacency: it reads 1/A of the bytes."""
        adj = adj.reshape(-1, adj.shape[-2], adj.shape[-1]).contiguous()
        B, E = adj.shape[0], adj.shape[-1]
        cap = int(cap if cap is not None else B * E * E)
        if cap > 2 ** 31 - 1:
            raise ValueError("edges_from_adj: cap %d does not fit the int32 ABI argument; pass an explicit cap (or use edges_from_adj_compact)" % cap)
        ei = torch.empty((2, cap), dtype=torch.int32, device=self.device)
        ea = torch.empty((cap,), dtype=torch.float32, device=self.device)
        ne = torch.zeros((1,), dtype=torch.int32, device=self.device)
        _lib.check(self.lib.gmpe_edges_from_adj(self.h, adj.data_ptr(), B, E, float(max_edge_dist), int(inclusive),
                                                ei.data_ptr(), ea.data_ptr(), cap, ne.data_ptr(), self._stream()),
                   "gmpe_edges_from_adj")
        m = int(ne.item())
        ei = ei[:, :min(m, cap)]
        return (ei.long() if index64 else ei), ea[:min(m, cap)], m

    def edges_from_adj_compact(self, adj_compact, copies, max_edge_dist, inclusive=False, cap=None, index64=True):
        """process_adj's edge set (gnn_new.py:329-358) for the [N*copies, E, E] batch the runner feeds the GNN, computed from the
        compact [N, E, E] adjacency: -> (edge_index [2, M] int64 (or int32), edge_attr [M], M)."""
        adj = adj_compact.reshape(-1, adj_compact.shape[-2], adj_compact.shape[-1]).contiguous()
        N, E = adj.shape[0], adj.shape[-1]
        ne = torch.zeros((1,), dtype=torch.int32, device=self.device)

        def run(ei, ea, cap):
            _lib.check(self.lib.gmpe_edges_from_adj_compact(self.h, adj.data_ptr(), N, int(copies), E, float(max_edge_dist), int(inclusive),
                                                            int(bool(index64)), ei.data_ptr(), ea.data_ptr(), cap, ne.data_ptr(), self._stream()),
                       "gmpe_edges_from_adj_compact")
            m = int(ne.item())
            if m >= 2 ** 31 - 1:
                raise _lib.GmpeError("edges_from_adj_compact: more than 2^31 - 2 edges (the count saturates, include/gmpe.h): split the batch")
            return m
        if cap is None and N * copies * E * E > 2 ** 28:
            # the worst case (every pair an edge) would be tens of GB at the big configs (c5 shard: 34 GB of int64 ids): size the buffers from a
            # count-only call (cap = 0 writes nothing) instead
            dummy = torch.empty((2,), dtype=torch.int64, device=self.device)
            cap = run(dummy, dummy, 0)
        cap = int(cap if cap is not None else N * copies * E * E)
        if cap == 0:
            # an empty edge set is a valid answer (max_edge_dist = 0, or every node masked): zero-size tensors have a null data_ptr the C ABI would
            # reject as a missing argument, so count with a one-element scratch and hand back empty tensors
            dummy = torch.empty((2,), dtype=torch.int64, device=self.device)
            m = run(dummy, dummy, 0)
            return (torch.empty((2, 0), dtype=torch.int64 if index64 else torch.int32, device=self.device),
                    torch.empty((0,), dtype=torch.float32, device=self.device), m)
        ei = torch.empty((2, cap), dtype=torch.int64 if index64 else torch.int32, device=self.device)
        ea = torch.empty((cap,), dtype=torch.float32, device=self.device)
        m = run(ei, ea, cap)
        return ei[:, :min(m, cap)], ea[:min(m, cap)], m

    def expand_node_obs(self, table, out=None, out_envs=None, env_offset=0):
        """node_obs rows from entity tables, bit-identical to what the engine writes (gmpe_expand_node_obs; module-level `expand_node_obs` needs no engine)."""
        return expand_node_obs(self.cfg, table, out=out, out_envs=out_envs, env_offset=env_offset)

    def expand_adj(self, table, copies=1, out=None, out_envs=None, env_offset=0):
        """The adjacency of every env-step from its entity table, bit-identical to the engine's own output (gmpe_expand_adj)."""
        return expand_adj(self.cfg, table, copies=copies, out=out, out_envs=out_envs, env_offset=env_offset)

    def masks_from_dones(self, done, masks, active_masks):
        """masks / active_masks (f32 [N,A,...], contiguous, N*A elements) from a uint8 [N,A] done tensor, one tiny kernel."""
        _lib.check(self.lib.gmpe_masks_from_dones(self.h, done.data_ptr(), masks.data_ptr() if masks is not None else None,
                                                  active_masks.data_ptr() if active_masks is not None else None, self._stream()),
                   "gmpe_masks_from_dones")

    # ------------------------------------------------------------------ timing hooks
    def timing(self, enable):
        _lib.check(self.lib.gmpe_timing_enable(self.h, int(bool(enable))), "gmpe_timing_enable")
        self._timing = bool(enable)                         # what a caller's graph capture asks before it records a step (gmpe.policy.CapturedRollout)

    def timing_read(self, reset=True):
        ms, n = C.c_double(), C.c_int64()
        _lib.check(self.lib.gmpe_timing_read(self.h, C.byref(ms), C.byref(n), int(reset)), "gmpe_timing_read")
        return ms.value, n.value

    def region_mark(self, which):
        """HIP event on the launch stream: which=0 before the first launch of a region, 1 after the last."""
        _lib.check(self.lib.gmpe_timing_mark(self.h, int(which), self._stream()), "gmpe_timing_mark")

    def region_ms(self):
        ms = C.c_double()
        _lib.check(self.lib.gmpe_timing_region_ms(self.h, C.byref(ms)), "gmpe_timing_region_ms")
        return ms.value

    @property
    def bytes_per_env_step(self):
        return algorithmic_bytes_per_env_step(self.cfg)


def _check_slots(name, t, numel, num_slots, stride):
    """The storage behind `t` holds num_slots slots of `numel` elements, `stride` elements apart, from t's first element on: what a rollout writes through it."""
    if stride < 0 or (t.storage_offset() + stride * (num_slots - 1) + numel) * t.element_size() > t.untyped_storage().nbytes():
        raise ValueError("%s: its storage does not hold %d slots of %d elements %d apart" % (name, num_slots, numel, stride))


def _expand(fn, cfg, table, out, out_envs, env_offset, row_shape, *extra):
    """What expand_node_obs and expand_adj share: check the tables, allocate or check `out` [..., out_envs, *row_shape], one launch of `fn` on the current stream."""
    lib = _lib.load()
    if table.dtype != torch.float64 or not table.is_contiguous() or not table.is_cuda or table.dim() < 2 or table.shape[-1] != cfg.entity_table_width:
        raise ValueError("table must be a contiguous float64 device tensor [..., n, %d]" % cfg.entity_table_width)
    n = int(table.shape[-2])
    blocks = int(table.numel() // (n * table.shape[-1])) if n else 0
    out_envs = n if out_envs is None else int(out_envs)
    shape = tuple(table.shape[:-2]) + (out_envs,) + tuple(row_shape)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=table.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != table.device:
        raise ValueError("out must be a contiguous float32 tensor of shape %s on %s" % (shape, table.device))
    if blocks and n:
        _lib.check(getattr(lib, fn)(C.byref(cfg), table.device.index, table.data_ptr(), blocks, n, out.data_ptr(), out_envs, int(env_offset), *extra,
                                    C.c_void_p(torch.cuda.current_stream(table.device).cuda_stream)), fn)
    return out


def expand_node_obs(cfg, table, out=None, out_envs=None, env_offset=0):
    """Learner side of the compact gather: float64 entity tables [..., n, W] (device tensor, contiguous; leading dims = blocks such as the T+1 slots of a rollout) ->
    node_obs float32 [..., out_envs, A, E, F], rows of the table's n envs written at env_offset .. env_offset + n of every block (default: out_envs = n). The rows are
    bit-identical to the engine's own node_obs (same arithmetic, gmpe_step.hip k_node_expand). No handle needed: the learner rank may own no envs."""
    return _expand("gmpe_expand_node_obs", cfg, table, out, out_envs, env_offset, (cfg.num_agents, cfg.num_entities, cfg.node_feats))


def expand_adj(cfg, table, copies=1, out=None, out_envs=None, env_offset=0):
    """float64 entity tables [..., n, W] -> adjacency float32 [..., out_envs, E, E] (copies = 1) or [..., out_envs, copies, E, E] (copies = A: the materialised
    per-agent form), rows of the table's n envs written at env_offset .. env_offset + n of every block. f32(sqrt(dx^2 + dy^2)) with the engine's own expression and
    this step's mask words: bit-identical to the adjacency the engine writes (gmpe_step.hip k_adj_from_table). No handle needed."""
    E = cfg.num_entities
    return _expand("gmpe_expand_adj", cfg, table, out, out_envs, env_offset, (E, E) if copies == 1 else (int(copies), E, E), int(copies))


# ---------------------------------------------------------------------- learner side of a rollout (gmpe_returns.hip)
def _stream_of(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _ordinal(dev):                                     # what the C entry points take
    return dev.index if dev.index is not None else torch.cuda.current_device()


def _dev_f32(name, t, shape, device, dtype=torch.float32):
    """`t` must be a contiguous `dtype` tensor of `shape` on `device`, else ValueError — checked before anything is launched (layout first, then device)."""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise ValueError("%s must be a contiguous %s tensor of shape %s" % (name, dtype, tuple(shape)))
    if t.device != device:
        raise ValueError("%s must be on %s (the device of the other arrays)" % (name, device))
    return t.data_ptr()


def _workspace(nbytes, workspace, dev):
    """`workspace` checked, or a fresh one of nbytes when None"""
    if workspace is None:
        return torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    if not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.device != dev or not workspace.is_contiguous() or \
            workspace.numel() < nbytes:
        raise ValueError("workspace must be a contiguous uint8 tensor of at least %d bytes on %s" % (nbytes, dev))
    return workspace


def _need_cuda(device):
    if device.type != "cuda":
        raise ValueError("the arrays must be CUDA (HIP) device tensors: these kernels have no CPU fallback")


def returns_workspace_bytes(lanes):
    """Device scratch (bytes) that compute_returns(..., normalized=...) needs for `lanes` = N*A lanes (gmpe_returns_workspace_bytes)."""
    n = C.c_size_t()
    _lib.check(_lib.load().gmpe_returns_workspace_bytes(int(lanes), C.byref(n)), "gmpe_returns_workspace_bytes")
    return int(n.value)


@torch.no_grad()
def denorm_scalars(value_normalizer, device):
    """(mean, sqrt(var)) of a ValueNorm (running_mean_var, onpolicy/utils/valuenorm.py:48-55) or a PopArt (debiased_mean_var,
    onpolicy/algorithms/utils/popart.py:101-106) as float32 [1] tensors on `device`. sqrt is taken where the normaliser keeps its statistics,
    as its own denormalize does (valuenorm.py:87-99), so x * std + mean has the reference's roundings. No host sync on a device normaliser."""
    f = getattr(value_normalizer, "running_mean_var", None) or getattr(value_normalizer, "debiased_mean_var", None)
    if f is None:
        raise TypeError("value_normalizer must have running_mean_var() (ValueNorm) or debiased_mean_var() (PopArt)")
    mean, var = f()
    std = torch.sqrt(var)
    if mean.numel() != 1 or std.numel() != 1:
        raise ValueError("the value normaliser must be scalar (input_shape 1, the runner's ValueNorm(1) / PopArt(..., 1))")
    cvt = lambda t: t.detach().reshape(1).to(device=device, dtype=torch.float32).contiguous()
    return cvt(mean), cvt(std)


def compute_returns(rewards, masks, value_preds, returns, next_value=None, gamma=0.99, gae_lambda=0.95, use_gae=True, use_proper_time_limits=False,
                    bad_masks=None, denorm=None, advantages=None, active_masks=None, normalized=None, workspace=None, advantages_only=False, shards=None):
    """GraphReplayBuffer.compute_returns (onpolicy/utils/graph_buffer.py:285-366) and the head of GR_MAPPO.train (graph_mappo.py:294-304) on the device,
    on the current stream, bit-identical to the reference's float32 NumPy for returns and raw advantages (gmpe_compute_returns).
      value_preds, returns, masks, bad_masks, active_masks: float32 [T+1, ...lane dims] (e.g. [T+1, N, A, 1]); rewards, advantages, normalized: [T, ...];
      next_value: float32 with one value per lane (e.g. [N, A, 1]); denorm: (mean, std) float32 [1] device tensors (denorm_scalars) or None.
    Side effects as the reference: with use_gae value_preds[T] = next_value, without it returns[T] = next_value. advantages (optional) receives
    returns[t] - denorm(value_preds[t]); normalized (optional, may be `advantages` itself) receives (adv - mean) / (std + 1e-5) over the entries with
    active_masks[t] != 0 — which needs `workspace` (uint8, returns_workspace_bytes(lanes) bytes; allocated here when None). advantages_only=True skips
    the recurrence and takes returns / value_preds as they stand (what train reads). Every argument is checked (ValueError) before the launch.
    shards: None, or the exchange of a data-parallel learner (gmpe.learner_shards): the arrays are this rank's lanes, and `normalized` (required then)
    is normalised by the mean / std over the lanes of ALL ranks, the same bits on every rank: compute_returns_begin, shards.exchange(.local),
    compute_returns_finish."""
    if shards is not None:
        from . import learner_shards
        learner_shards.check_shards(shards)
        h = compute_returns_begin(rewards, masks, value_preds, returns, next_value, gamma, gae_lambda, use_gae, use_proper_time_limits, bad_masks, denorm,
                                  advantages, active_masks, normalized, workspace, advantages_only)
        return compute_returns_finish(h, learner_shards.gather(shards, h.local, "compute_returns"))
    plan, dev, _ = _returns_plan(rewards, masks, value_preds, returns, next_value, gamma, gae_lambda, use_gae, use_proper_time_limits, bad_masks, denorm,
                                 advantages, active_masks, normalized, workspace, advantages_only)
    _need_cuda(dev)
    _lib.check(_lib.load().gmpe_compute_returns(dev.index, C.byref(plan), _stream_of(dev)), "gmpe_compute_returns")
    return returns


def _returns_plan(rewards, masks, value_preds, returns, next_value, gamma, gae_lambda, use_gae, use_proper_time_limits, bad_masks, denorm, advantages,
                  active_masks, normalized, workspace, advantages_only):
    """The checked arguments of compute_returns as a gmpe_returns_plan -> (plan, device, the tensors the plan points to)."""
    if not isinstance(value_preds, torch.Tensor) or value_preds.dim() < 1 or value_preds.shape[0] < 2:
        raise ValueError("value_preds must be a float32 tensor [T+1, ...] with T >= 1")
    dev = value_preds.device
    T1 = int(value_preds.shape[0])
    slot = tuple(value_preds.shape[1:])
    lanes = int(np.prod(slot, dtype=np.int64))
    full, half = (T1,) + slot, (T1 - 1,) + slot
    if lanes < 1:
        raise ValueError("value_preds has no lanes")
    ptr = lambda name, t, shape: None if t is None else _dev_f32(name, t, shape, dev)
    for name, t in (("returns", returns),) + (() if advantages_only else (("rewards", rewards), ("masks", masks), ("next_value", next_value))):
        if t is None:
            raise ValueError("%s is required" % name)
    if use_proper_time_limits and not advantages_only and bad_masks is None:
        raise ValueError("use_proper_time_limits needs bad_masks")
    if advantages_only and advantages is None and normalized is None:
        raise ValueError("advantages_only needs advantages or normalized")
    if normalized is not None and active_masks is None:
        raise ValueError("normalized advantages need active_masks")
    plan = _lib.GmpeReturnsPlan()
    plan.num_steps, plan.lanes, plan.stride = T1 - 1, lanes, lanes
    plan.flags = (_lib.RETURNS_GAE if use_gae else 0) | (_lib.RETURNS_PROPER_TIME_LIMITS if use_proper_time_limits else 0) | \
                 (_lib.RETURNS_ADVANTAGES_ONLY if advantages_only else 0)
    plan.gamma, plan.gae_lambda = float(gamma), float(gae_lambda)
    plan.value_preds, plan.returns = ptr("value_preds", value_preds, full), ptr("returns", returns, full)
    if not advantages_only:
        plan.rewards, plan.masks = ptr("rewards", rewards, half), ptr("masks", masks, full)
        if not isinstance(next_value, torch.Tensor) or next_value.numel() != lanes:
            raise ValueError("next_value must hold one value per lane (%d)" % lanes)
        plan.next_value = ptr("next_value", next_value, tuple(next_value.shape))
        if use_proper_time_limits:
            plan.bad_masks = ptr("bad_masks", bad_masks, full)
    if denorm is not None:
        if len(denorm) != 2:
            raise ValueError("denorm must be a (mean, std) pair")
        plan.denorm_mean, plan.denorm_std = ptr("denorm mean", denorm[0], (1,)), ptr("denorm std", denorm[1], (1,))
    plan.advantages = ptr("advantages", advantages, half)
    if normalized is not None:
        plan.normalized = ptr("normalized", normalized, half)
        plan.active_masks = ptr("active_masks", active_masks, full)
        workspace = _workspace(returns_workspace_bytes(lanes), workspace, dev)
        plan.workspace, plan.workspace_bytes = workspace.data_ptr(), workspace.numel()
    return plan, dev, (rewards, masks, value_preds, returns, next_value, bad_masks, denorm, advantages, active_masks, normalized, workspace)


class ReturnsShard(object):
    """What compute_returns_begin leaves for compute_returns_finish: `.local`, this shard's (n, mean, M2) of the active raw advantages as an f64 [3]
    device tensor (valid once the stream reaches it), and everything the plan points to, kept alive until finish has enqueued its launches."""

    def __init__(self, plan, device, keep, returns, local):
        self.plan, self.device, self.keep, self.returns, self.local, self.done = plan, device, keep, returns, local, False


def compute_returns_begin(rewards, masks, value_preds, returns, next_value=None, gamma=0.99, gae_lambda=0.95, use_gae=True, use_proper_time_limits=False,
                          bad_masks=None, denorm=None, advantages=None, active_masks=None, normalized=None, workspace=None, advantages_only=False):
    """The first phase of compute_returns over one shard of a batch (gmpe_compute_returns_shard, GMPE_SHARD_LOCAL), same arguments: returns, side
    effects and raw advantages are written as compute_returns writes them (they are lane-local), the shard's advantage statistics go to the handle's
    `.local` in compute_returns' own merge order, and nothing is normalised yet: the raw advantages wait in `advantages` (in `normalized` when
    advantages is None). `normalized` and `active_masks` are required. -> ReturnsShard"""
    if normalized is None:
        raise ValueError("a sharded compute_returns exchanges the statistics of the normalised advantages: normalized (and active_masks) are required")
    plan, dev, keep = _returns_plan(rewards, masks, value_preds, returns, next_value, gamma, gae_lambda, use_gae, use_proper_time_limits, bad_masks, denorm,
                                    advantages, active_masks, normalized, workspace, advantages_only)
    from . import learner_shards
    sp = _lib.GmpeReturnsShardPlan()
    local = learner_shards.begin("gmpe_compute_returns_shard", sp, plan, _lib.RETURNS_SHARD_STATS, dev)
    return ReturnsShard(sp, dev, keep, returns, local)


def compute_returns_finish(handle, all_stats):
    """The second phase (GMPE_SHARD_APPLY): all_stats f64 [world, 3], row r = shard r's `.local` (torch.stack of the handles' .local in one process,
    an all-gather across ranks). The rows are merged as a left fold in index order, an empty shard (n = 0) changing nothing, and this shard's raw
    advantages are normalised by the result — the statistics of the whole batch, the same bits on every shard. Once per handle. -> returns"""
    from . import learner_shards
    if not isinstance(handle, ReturnsShard):
        raise TypeError("handle must come from compute_returns_begin")
    learner_shards.finish("gmpe_compute_returns_shard", handle, handle.device, all_stats, "compute_returns_finish",
                          "compute_returns_finish was already called on this handle (in place it would normalise twice)")
    return handle.returns


def available_actions_from_dones(dones, out, first=0, count=None):
    """The available_actions of the shipped training loop (graph_mpe_runner.py:73-141 collect_with_mask + get_finished, stored at slot step + 1 by
    GraphReplayBuffer.insert) for the positions t = (first + k) % T, k < count (default: first .. T - 1), one launch on the current stream:
    out[t] = ones at t = 0; for t >= 1 a one-hot "stop" row at n_actions // 2 for every agent done at step t - 1 (dones[t - 1]), ones otherwise.
      dones: uint8 / bool [T, ...lane dims] (a rollout buffer's dones); out: float32 [T, ...lane dims, n_actions] (a buffer's available_actions[1:])."""
    if not isinstance(dones, torch.Tensor) or dones.dtype not in (torch.uint8, torch.bool) or not dones.is_contiguous() or dones.dim() < 2:
        raise ValueError("dones must be a contiguous uint8 / bool tensor [T, ...]")
    dev = dones.device
    T = int(dones.shape[0])
    if not isinstance(out, torch.Tensor) or out.dim() != dones.dim() + 1:
        raise ValueError("out must be a float32 tensor [T, ..., n_actions] matching dones")
    n = int(out.shape[-1])
    _dev_f32("out", out, tuple(dones.shape) + (n,), dev)
    lanes = int(dones[0].numel())
    count = T - int(first) if count is None else int(count)
    if not 0 <= int(first) < T or count < 0 or n < 1 or lanes < 1:
        raise ValueError("need 0 <= first < T, count >= 0, n_actions >= 1 and at least one lane")
    _need_cuda(dev)
    plan = _lib.GmpeAvailPlan(dones.data_ptr(), out.data_ptr(), lanes, n, T, int(first), count, lanes, lanes * n)
    _lib.check(_lib.load().gmpe_available_actions_from_dones(dev.index, C.byref(plan), _stream_of(dev)), "gmpe_available_actions_from_dones")
    return out


# ---------------------------------------------------------------------- the learner's fields of a rollout step (gmpe_learner.hip)
# input name -> (buffer array, whether it has slot T, dtypes the input may have)
LEARNER_INPUTS = dict(values=("value_preds", True, (torch.float32,)), actions=("actions", False, (torch.int64, torch.float32)),
                      action_log_probs=("action_log_probs", False, (torch.float32,)), rnn_states=("rnn_states", True, (torch.float32,)),
                      rnn_states_critic=("rnn_states_critic", True, (torch.float32,)))


def _slots(name, t, lead, tail_dim, dev):
    """A buffer array [S, *lead, *tail] (tail_dim trailing dims): float32 on `dev`, each slot contiguous, slots stride(0) elements apart; returns the tail."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 1 + len(lead) + tail_dim or tuple(t.shape[1:1 + len(lead)]) != lead:
        raise ValueError("%s must be a float32 tensor [slots, %s, ...] with %d trailing dims" % (name, ", ".join(str(x) for x in lead), tail_dim))
    if not t[0].is_contiguous() or t.stride(0) < t[0].numel():
        raise ValueError("%s: every slot must be contiguous and the slots must not overlap" % name)
    if t.device != dev:
        raise ValueError("%s must be on %s (the device of the other arrays)" % (name, dev))
    return tuple(int(x) for x in t.shape[1 + len(lead):])


def _learner_plan(plan, step, dones, arrays, given):
    """insert_learner's checks, shared with step_tail: fills the gmpe_learner_plan `plan` -> (the inputs to keep alive, device, T, lead dims, lanes)"""
    if not isinstance(dones, torch.Tensor) or dones.dtype not in (torch.uint8, torch.bool) or dones.dim() < 2 or not dones[0].is_contiguous():
        raise ValueError("dones must be a uint8 / bool tensor [T, ...] with contiguous slots")
    dev = dones.device
    T, lead = int(dones.shape[0]), tuple(int(x) for x in dones.shape[1:])
    lanes = int(np.prod(lead, dtype=np.int64))
    if not 0 <= int(step) < T or lanes < 1:
        raise ValueError("need 0 <= step < T = %d and at least one lane" % T)
    unknown = set(arrays) - {v[0] for v in LEARNER_INPUTS.values()}
    if unknown:
        raise ValueError("unknown learner arrays: %s" % sorted(unknown))
    plan.lanes, plan.t, plan.num_steps = lanes, int(step), T
    plan.dones, plan.stride_dones = dones.data_ptr(), dones.stride(0)
    plan.recurrent_n, plan.hidden, plan.hidden_critic, plan.act_dim = 1, 1, 1, 1
    keep = []
    for name, x in given.items():
        if x is None:
            continue
        out, has_last, dtypes = LEARNER_INPUTS[name]
        buf = arrays.get(out)
        if buf is None:
            raise ValueError("%s given without the %s array it goes to" % (name, out))
        tail = _slots(out, buf, lead, 2 if name.startswith("rnn") else 1, dev)
        if buf.shape[0] != T + (1 if has_last else 0):
            raise ValueError("%s must hold %d slots (T = %d)" % (out, T + (1 if has_last else 0), T))
        if not isinstance(x, torch.Tensor) or x.dtype not in dtypes or not x.is_contiguous() or x.numel() != lanes * int(np.prod(tail)) or \
                (name != "values" and tuple(x.shape[-len(tail):]) != tail):
            raise ValueError("%s must be a contiguous %s tensor [%d, %s]" % (name, "/".join(str(d) for d in dtypes), lanes, ", ".join(map(str, tail))))
        if x.device != dev:
            raise ValueError("%s must be on %s (the device of the other arrays)" % (name, dev))
        keep.append(x)
        if name == "values":
            plan.values, plan.value_preds, plan.stride_value_preds = x.data_ptr(), buf.data_ptr(), buf.stride(0)
        elif name == "actions":
            plan.actions_in, plan.actions, plan.stride_actions = x.data_ptr(), buf.data_ptr(), buf.stride(0)
            plan.actions_int64, plan.act_dim = int(x.dtype == torch.int64), tail[0]
        elif name == "action_log_probs":
            plan.log_probs_in, plan.action_log_probs, plan.stride_action_log_probs = x.data_ptr(), buf.data_ptr(), buf.stride(0)
            plan.act_dim = tail[0]
        elif name == "rnn_states":
            plan.rnn_in, plan.rnn_states, plan.stride_rnn_states = x.data_ptr(), buf.data_ptr(), buf.stride(0)
            plan.recurrent_n, plan.hidden = tail
        else:
            plan.rnn_critic_in, plan.rnn_states_critic, plan.stride_rnn_states_critic = x.data_ptr(), buf.data_ptr(), buf.stride(0)
            plan.recurrent_n, plan.hidden_critic = tail
    if given["actions"] is not None and given["action_log_probs"] is not None and arrays["actions"].shape[-1] != arrays["action_log_probs"].shape[-1]:
        raise ValueError("actions and action_log_probs must have the same last dim")
    if given["rnn_states"] is not None and given["rnn_states_critic"] is not None and \
            arrays["rnn_states"].shape[-2] != arrays["rnn_states_critic"].shape[-2]:
        raise ValueError("rnn_states and rnn_states_critic must have the same recurrent_N")
    return keep, dev, T, lead, lanes


def insert_learner(step, dones, arrays, values=None, actions=None, action_log_probs=None, rnn_states=None, rnn_states_critic=None):
    """GMPERunner.insert's learner fields of step `step` (graph_mpe_runner.py:384-392 + graph_buffer.py:229-234) as one launch on the current stream
    (gmpe_insert_learner): value_preds[step] = values, actions[step] = float32(actions), action_log_probs[step] = action_log_probs, and
    rnn_states[step + 1] / rnn_states_critic[step + 1] = the policy's states with the rows of every agent done at `step` (dones[step] != 0) zeroed.
      dones: uint8 / bool [T, N, A] (each slot contiguous; slot `step` is read on the device, no host sync);
      arrays: dict of the buffer's arrays, some of value_preds [T+1, N, A, 1], actions / action_log_probs [T, N, A, k],
              rnn_states / rnn_states_critic [T+1, N, A, R, H] (float32; each slot contiguous, any stride(0) of at least one slot: views of a slab);
      inputs: the policy's outputs as contiguous device tensors with N*A rows — values f32 [N*A, 1], actions int64 (what the policy returns) or f32
              [N*A, k], action_log_probs f32 [N*A, k], rnn_states / rnn_states_critic f32 [N*A, R, H]. None skips a field.
    Every argument is checked (ValueError) before the launch."""
    given = dict(values=values, actions=actions, action_log_probs=action_log_probs, rnn_states=rnn_states, rnn_states_critic=rnn_states_critic)
    plan = _lib.GmpeLearnerPlan()
    keep, dev = _learner_plan(plan, step, dones, arrays, given)[:2]
    if not keep:
        return
    _need_cuda(dev)
    _lib.check(_lib.load().gmpe_insert_learner(dev.index, C.byref(plan), _stream_of(dev)), "gmpe_insert_learner")


def step_tail(step, dones, arrays, *, num_agents, masks=None, active_masks=None, available_actions=None, draw_dev=None, draw_inc=0, values=None,
              actions=None, action_log_probs=None, rnn_states=None, rnn_states_critic=None):
    """Everything that follows the env step of step `step` as ONE launch on the current stream (gmpe_step_tail): insert_learner(step, dones, arrays, ...)
    for whatever inputs are given (none is fine), masks[step + 1] / active_masks[step + 1] from dones[step] (masks_from_dones' rule, lane q of env
    q // num_agents), the stop rows available_actions_from_dones writes for position `step` — available_actions[step + 1], from dones[step - 1], all
    ones at step 0 —, and draw_dev += draw_inc. Bit for bit what the separate calls write; the launch is made also when only the masks are asked for.
      dones, arrays and the inputs: as for insert_learner. masks / active_masks: float32 [T+1, ...lane dims(, 1)]; available_actions: float32
      [T+1, ...lane dims, n_actions] (the buffer's whole array); each slot contiguous, any stride(0) of at least one slot. draw_dev: the int64 [1]
      device counter of act_head / sample_actions, called with draw_inc=0 for this step, or None."""
    given = dict(values=values, actions=actions, action_log_probs=action_log_probs, rnn_states=rnn_states, rnn_states_critic=rnn_states_critic)
    tp = _lib.GmpeStepTailPlan()
    keep, dev, T, lead, lanes = _learner_plan(tp.learner, step, dones, arrays, given)
    if int(num_agents) < 1 or lanes % int(num_agents):
        raise ValueError("need num_agents >= 1 dividing the %d lanes" % lanes)
    tp.num_agents = int(num_agents)
    for name, x in (("masks", masks), ("active_masks", active_masks), ("available_actions", available_actions)):
        if x is None:
            continue
        avail = name == "available_actions"
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() < 1 + len(lead) + avail or x.shape[0] != T + 1 or \
                tuple(x.shape[1:1 + len(lead)]) != lead or (not avail and x[0].numel() != lanes) or x.dim() > 2 + len(lead):
            raise ValueError("%s must be a float32 tensor [%d, %s%s]" % (name, T + 1, ", ".join(map(str, lead)), ", n_actions" if avail else "(, 1)"))
        if not x[0].is_contiguous() or x.stride(0) < x[0].numel():
            raise ValueError("%s: every slot must be contiguous and the slots must not overlap" % name)
        if x.device != dev:
            raise ValueError("%s must be on %s (the device of the other arrays)" % (name, dev))
        if avail:
            n = int(x.shape[-1])
            if not 1 <= n <= 64:
                raise ValueError("available_actions: n_actions must be in 1 .. 64")
            tp.n_actions, tp.available_actions, tp.stride_available_actions = n, x[1].data_ptr(), x.stride(0)
        else:
            setattr(tp, name, x.data_ptr())
            setattr(tp, "stride_" + name, x.stride(0))
    if int(draw_inc) < 0:
        raise ValueError("draw_inc must be >= 0")
    if draw_dev is not None:
        if not isinstance(draw_dev, torch.Tensor) or draw_dev.dtype not in (torch.int64, torch.uint64) or draw_dev.numel() != 1 or \
                not draw_dev.is_contiguous():
            raise ValueError("draw_dev must be a contiguous int64 tensor with one element")
        if draw_dev.device != dev:
            raise ValueError("draw_dev must be on %s (the device of the other arrays)" % dev)
        tp.draw_dev, tp.draw_inc = draw_dev.data_ptr(), int(draw_inc) & 0xFFFFFFFFFFFFFFFF
    _need_cuda(dev)
    _lib.check(_lib.load().gmpe_step_tail(dev.index, C.byref(tp), _stream_of(dev)), "gmpe_step_tail")
