"""BatchedGraphMPEVecEnv — same surface as GraphSubprocVecEnv, backed by the HIP engine.

Mirrors onpolicy/envs/env_wrappers.py:959-1037 (class GraphSubprocVecEnv) and its base ShareVecEnv
(:28-141): `num_envs`, the eight space lists, `reset(num_current_episode)`,
`step_async/step_wait/step(actions, num_current_episode)`, `close()`, `render()`.
Where the reference forks N processes that each run MultiAgentGraphEnv.step
(multiagent/environment.py:1021-1063) and ship pickled fp64 arrays through pipes, this class makes
ONE kernel launch per step for all N envs and hands the runner NumPy views in the dtypes its
buffer stores (float32 / int32 / bool; onpolicy/utils/graph_buffer.py:84-114).
"""
import functools

import numpy as np
import torch

from . import _lib
from .config import INFO_KEYS, NODE_FEATS, ROT_FAMILY, config_from_args
from .engine import GmpeEngine, StepOutputs
from .sharding import shard_range
from .spaces import Box, Discrete


class LazyInfos(object):
    """Sequence of N per-env info lists, materialised from the device counters only when read.

    The runner touches infos only every `log_interval` episodes (graph_mpe_runner.py:166-189,
    base_runner.py:194-290: `for info in infos: info[agent_id][key]`); building 4096x10 dicts of 17
    keys every step would dominate the host, so the dicts are created on first access.
    """

    def __init__(self, info_dev, n_envs, n_agents, include_min_time=True, include_phase=False, owner=None, generation=0):
        """info_dev: the device tensor the step wrote its info rows into. The vec env alternates TWO such tensors (no per-step clone), so
        the rows stay valid until the step after next; `owner` / `generation` let a late read fail loudly instead of returning a later
        step's rows."""
        self._dev = info_dev
        self._host = None
        self._n, self._a = n_envs, n_agents
        self._owner, self._gen = owner, generation
        # (key, column) pairs: 'Min_time_to_goal' only with max_speed (…_july.py:826-828), 'Phase_reached' only in rot_inv (:835)
        self._keys = [(k, j) for j, k in enumerate(INFO_KEYS)
                      if (k != "Min_time_to_goal" or include_min_time) and (k != "Phase_reached" or include_phase)]

    def _fetch(self):
        if self._host is None:
            if self._owner is not None and self._owner._info_gen - self._gen >= 2:
                raise RuntimeError("infos of step %d read after step %d overwrote their device buffer: read infos (or call .as_array()) "
                                   "before the step after next" % (self._gen, self._owner._info_gen))
            self._host = self._dev.detach().cpu().numpy().astype(np.float64)
            self._dev = None
        return self._host

    def __len__(self):
        return self._n

    def __getitem__(self, e):
        if isinstance(e, slice):
            return [self[i] for i in range(*e.indices(self._n))]
        if e < 0:
            e += self._n
        if not 0 <= e < self._n:
            raise IndexError(e)
        h = self._fetch()
        return [{k: float(h[e, a, j]) for k, j in self._keys} for a in range(self._a)]

    def __iter__(self):
        for e in range(self._n):
            yield self[e]

    def as_array(self):
        """[N, A, 18] float64 in config.INFO_KEYS order (no dict construction)."""
        return self._fetch()


_KEYS = {False: ("obs", "agent_id", "node_obs", "adj"), True: ("obs", "agent_id", "node_obs", "adj", "reward", "done")}   # reset / step hand-off


def _check_actions(actions, N, A, n_actions):
    """The runner's actions (NumPy or tensor) -> (array, "onehot" | "index"), refused with ValueError unless [N, A, n_actions] or [N, A]."""
    a = actions if torch.is_tensor(actions) else np.asarray(actions)
    if a.ndim == 3:
        if tuple(a.shape) != (N, A, n_actions):
            raise ValueError("actions must be [N=%d, A=%d, %d]" % (N, A, n_actions))
        return a, "onehot"
    if a.ndim == 2:
        if tuple(a.shape) != (N, A):
            raise ValueError("actions must be [N=%d, A=%d]" % (N, A))
        return a, "index"
    raise ValueError("actions must be a one-hot [N,A,n_act] or an index [N,A] array")


def _expand_adj(a, num_agents, compact):
    """The compact [N, E, E] adjacency as the runner's [N, A, E, E] (a zero-copy broadcast view); a materialised one is returned as is."""
    if compact:
        N, E = a.shape[0], a.shape[-1]
        a = np.broadcast_to(a[:, None], (N, num_agents, E, E))
    return a


class BatchedGraphMPEVecEnv(object):
    """Drop-in for GraphSubprocVecEnv([get_env_fn(i) for i in range(n_rollout_threads)])."""
    closed = False
    viewer = None
    metadata = {"render.modes": ["human", "rgb_array"]}

    def __init__(self, all_args, num_envs=None, device=0, env_id_base=0, adj_broadcast_view=True, pinned_host=True, safety_filter=None,
                 eval_surface=False, _host=None):
        """eval_surface: reproduce GraphDummyVecEnv instead (env_wrappers.py:903-956) — what train_mpe.py:36, 61 / eval_mpe.py:36 pick for
        n_rollout_threads == 1 and GMPERunner.render unpacks (graph_mpe_runner.py:621-622): `step` returns an 8-tuple whose last element is
        `reset_count` (1 if an env of the batch was auto-reset in this step, else 0; env_wrappers.py:923-936).
        safety_filter: the hook slot of `World.step`'s safety filter (multiagent/core.py:692-736). A callable
        `f(engine, actions_dev) -> (ctrl [N,A,2] float64 device tensor, use [N,A] uint8 device tensor or None)` called before every
        step; where `use` is set the engine integrates `ctrl` instead of the decoded action. The HJ / CBF filter of the reference
        (safety_filter.py: jax / cvxpy / value-function data) is not built, so `args.use_safety_filter` without a callable raises.
        _host (private): two caller-owned sets of host destinations (dicts obs / agent_id / node_obs / adj / reward / done / err of CPU tensors with this
        handle's shapes) used instead of allocating its own — how MultiDeviceGraphMPEVecEnv gives each shard its row range of one [N, ...] array per output."""
        if getattr(all_args, "use_safety_filter", False) and safety_filter is None:
            raise NotImplementedError("use_safety_filter=True: the HJ/CBF filter is out of scope (DESIGN.md); pass safety_filter=callable "
                                      "to fill the hook slot")
        self._safety_filter = safety_filter
        self._eval_surface = bool(eval_surface)
        self.cfg = config_from_args(all_args, num_envs=num_envs, env_id_base=env_id_base)
        # The reference's per-agent adj arrays alias ONE E x E matrix per env, so the
        # engine writes that matrix once and the [N,A,E,E] result is a zero-copy broadcast view.
        self._compact = bool(adj_broadcast_view)
        self.engine = self._make_engine(self.cfg, device)
        c = self.cfg
        self.num_envs = c.num_envs
        self.num_agents = self.n = c.num_agents
        A, E, D = c.num_agents, c.num_entities, c.obs_dim
        f32 = np.float32
        # spaces: multiagent/environment.py:152-208 (obs/share_obs/action) and :986-1018 (graph)
        self.observation_space = [Box(-np.inf, np.inf, (D,), f32) for _ in range(A)]
        self.share_observation_space = [Box(-np.inf, np.inf, (A * D,), f32) for _ in range(A)]
        self.action_space = [Discrete(c.n_actions) for _ in range(A)]
        self.node_observation_space = [Box(-np.inf, np.inf, (E, self.cfg.node_feats), f32) for _ in range(A)]
        self.adj_observation_space = [Box(-np.inf, np.inf, (E, E), f32) for _ in range(A)]
        self.edge_observation_space = [Box(-np.inf, np.inf, (1,), f32) for _ in range(A)]
        self.agent_id_observation_space = [Box(-np.inf, np.inf, (1,), f32) for _ in range(A)]
        self.share_agent_id_observation_space = [Box(-np.inf, np.inf, (A * 1,), f32) for _ in range(A)]
        self.waiting = False
        self._pending = None
        self._errors_reported = False
        # info rows: two device buffers bound alternately (a LazyInfos keeps a reference to its step's buffer instead of a per-step clone);
        # sticky device error flags (tape exhausted / placement gave up) travel down with every hand-off and raise GmpeError here
        o = self.engine.out
        self._outs = [o, StepOutputs(**{k: (torch.empty_like(o.info) if k == "info" else getattr(o, k)) for k in StepOutputs.__slots__})]
        self._info_gen = 0
        self._err_dev = self.engine.state_tensor("error_flags")
        # Host hand-off for the NumPy runner: two alternating sets of pinned staging buffers, filled by asynchronous
        # D2H copies on the engine's stream (arrays returned by step t stay valid until step t+2; the runner copies
        # them into its replay buffer immediately, graph_buffer.py:223-236). pinned_host=False returns fresh arrays.
        self._pinned = bool(pinned_host)
        self._host = _host
        self._flip = 0
        if self._pinned and self._host is None:
            o = self.engine.out
            mk = lambda t: self._empty_host(t.shape, t.dtype, True)
            self._host = [dict(obs=mk(o.obs), agent_id=mk(o.agent_id), node_obs=mk(o.node_obs), adj=mk(o.adj),
                               reward=mk(o.reward), done=mk(o.done), err=mk(self._err_dev)) for _ in range(2)]
        # Actions go up through pinned staging too: whatever dtype the runner hands over (np.eye(n)[a] is float64, indices are int64) is
        # converted straight INTO the pinned buffer (single-threaded NumPy, see _upload) and uploaded from there.
        dev = self.engine.device
        self._act_host = dict(onehot=self._empty_host((c.num_envs, A, c.n_actions), torch.float32, self._pinned),
                              index=self._empty_host((c.num_envs, A), torch.int32, self._pinned))
        self._act_dev = dict(onehot=torch.empty((c.num_envs, A, c.n_actions), dtype=torch.float32, device=dev),
                             index=torch.empty((c.num_envs, A), dtype=torch.int32, device=dev))

    # ------------------------------------------------------------------ helpers
    def _make_engine(self, cfg, device):
        return GmpeEngine(cfg, device=device, adj_compact=self._compact, with_info=True)

    @staticmethod
    def _empty_host(shape, dtype, pinned):
        return torch.empty(tuple(shape), dtype=dtype, device="cpu", pin_memory=pinned)

    def _sync(self):
        torch.cuda.current_stream(self.engine.device).synchronize()

    def _issue(self, o, keys, dst):
        """Queue the D2H copies of outputs `keys` of `o` and of the error flags into the host tensors `dst` (asynchronous into pinned memory; on the
        engine's current stream)."""
        for k in keys:
            dst[k].copy_(getattr(o, k), non_blocking=True)
        dst["err"].copy_(self._err_dev, non_blocking=True)

    def _fetch(self, o, with_step_outputs):
        """Device outputs -> NumPy. Returns (obs, agent_id, node_obs, adj[, reward, done])."""
        keys = _KEYS[with_step_outputs]
        if self._pinned:
            h = self._host[self._flip]
            self._flip ^= 1
            self._issue(o, keys, h)
            self._sync()
            arrs = [h[k].numpy() for k in keys]
            err = h["err"].numpy()
        else:
            arrs = [getattr(o, k).detach().cpu().numpy() for k in keys]
            err = self._err_dev.cpu().numpy()
        if err.any():
            self._raise_errors()
        arrs[3] = _expand_adj(arrs[3], self.num_agents, self._compact)
        return arrs

    def _raise_errors(self):
        """Sticky per-env error flags of the engine (include/gmpe.h error_flags) -> GmpeError. The reference has no counterpart: its
        rejection sampler spins forever in a world too small for its agents (…_july.py:462-486), the engine's is bounded."""
        self._errors_reported = True                  # close() will not raise the same sticky flags again
        self.engine.check_errors()

    # ------------------------------------------------------------------ GraphSubprocVecEnv surface
    def reset(self, num_current_episode=0):
        """-> (obs [N,A,D], agent_id [N,A,1], node_obs [N,A,E,F], adj [N,A,E,E])  (env_wrappers.py:1006-1013)"""
        o = self.engine.reset()
        return tuple(self._fetch(o, False))

    def step_async(self, actions, num_current_episode=None):
        """actions: [N, A, n_actions] one-hot (graph_mpe_runner.py:375-377), or [N, A] integer indices."""
        if self.waiting:
            raise RuntimeError("step_async called while a step is pending")
        a, kind = _check_actions(actions, self.num_envs, self.num_agents, self.cfg.n_actions)
        self._pending = self._launch(a, kind)
        self.waiting = True

    def _launch(self, a, kind):
        """Checked actions of this handle's envs -> upload, safety filter, one launch on the current stream. Returns the outputs it writes."""
        t = self._upload(a, kind)
        self._filter(t)
        self._next_info()
        return self.engine.step_onehot(t) if kind == "onehot" else self.engine.step(t)

    def _next_info(self):
        self._info_gen += 1
        self.engine.rebind(self._outs[self._info_gen & 1])

    def _upload(self, a, kind):
        """Host (NumPy / CPU tensor, any numeric dtype) or device actions -> the engine's device tensor of the right dtype."""
        dst = self._act_dev[kind]
        if torch.is_tensor(a) and a.is_cuda:
            return a if (a.dtype == dst.dtype and a.is_contiguous() and a.device == dst.device) else dst.copy_(a)
        stage = self._act_host[kind]
        # dtype conversion straight into pinned memory — with NumPy on purpose: a torch CPU op of this size fans out over every host
        # core (128 OpenMP threads on the MI355X boxes), and under a CPU quota their spin-waiting gets the whole process throttled for the
        # rest of the scheduler period (~90 ms stalls once per ~30 steps, tools/hostpath3.py)
        np.copyto(stage.numpy(), a.numpy() if torch.is_tensor(a) else a, casting="unsafe")
        return dst.copy_(stage, non_blocking=True)

    def _filter(self, actions_dev):
        if self._safety_filter is not None:
            ctrl, use = self._safety_filter(self.engine, actions_dev)
            self.engine.set_control_override(ctrl, use)

    def step_wait(self):
        """-> 7-tuple (obs, agent_id, node_obs, adj, rewards [N,A], dones [N,A] bool, infos)
        (env_wrappers.py:996-1004). Envs whose agents were all done carry POST-reset observations with
        the terminal reward/done (graphworker, env_wrappers.py:865-873)."""
        if not self.waiting:
            raise RuntimeError("step_wait without step_async")
        o = self._pending
        self._pending, self.waiting = None, False
        obs, ids, node, adj, rew, done = self._fetch(o, True)    # synchronises the stream
        done = done.astype(bool)
        if self.cfg.collaborative:
            rew = rew[..., None]                       # `reward_n = [[reward]] * self.n` (environment.py:1056-1061) stacks to [N, A, 1]
        # 'Phase_reached' is an info key of the rot_inv family only (rot_inv.py:835); the July file's info_callback has 17 keys (…_july.py:806-828)
        infos = self._infos(o)
        if self._eval_surface:
            reset_count = 1 if done.all(axis=1).any() else 0       # GraphDummyVecEnv.step_wait (env_wrappers.py:923-936)
            return obs, ids, node, adj, rew, done, infos, reset_count
        return obs, ids, node, adj, rew, done, infos

    def _infos(self, o):
        return LazyInfos(o.info, self.num_envs, self.num_agents, include_min_time=self.cfg.max_speed > 0,
                         include_phase=self.cfg.scenario in ROT_FAMILY, owner=self, generation=self._info_gen)

    def step(self, actions, num_current_episode=None):
        self.step_async(actions, num_current_episode)
        return self.step_wait()

    def reset_task(self):
        raise NotImplementedError("reset_task is not part of the GraphMPE path")

    def render(self, mode="rgb_array"):
        raise NotImplementedError("rendering (pyglet viewer) is out of scope of the step engine")

    def close(self):
        """Frees the handle unconditionally. Sticky device errors that no reset / step hand-off has raised yet are raised here — once: a close() in a
        `finally` / `except` clean-up path after a GmpeError must not replace the exception that is already propagating (it warns instead)."""
        if self.closed:
            return
        try:
            if not self._errors_reported:
                self.engine.check_errors()            # last chance to report sticky device errors (synchronises)
        except _lib.GmpeError:
            self._errors_reported = True
            raise
        except Exception as e:                        # a handle that is already in a failed state: do not mask the original failure
            import warnings
            warnings.warn("BatchedGraphMPEVecEnv.close: could not read the device error flags (%s)" % e)
        finally:
            self.engine.close()
            self.closed = True

    @property
    def unwrapped(self):
        return self

    # ------------------------------------------------------------------ extras (not in the reference)
    def step_device(self, action_idx):
        """Zero-copy variant: int32 device tensor in, device tensors out (engine.StepOutputs)."""
        return self.engine.step(action_idx)

    def seed(self, seed=None):
        raise NotImplementedError("seeds are part of the config (args.seed): per-env streams are keyed by "
                                  "(seed, env id), the counterpart of env.seed(seed + rank*1000) in train_mpe.py:31")


def _keeps_current_device(fn):
    """libgmpe's entry points hipSetDevice to their handle's device and leave it set: restore the caller's current device after the shards' calls, so a
    runner's `device="cuda"` allocations do not move to the last shard's device."""
    @functools.wraps(fn)
    def wrapper(self, *args, **kw):
        prev = torch.cuda.current_device() if torch.cuda.is_initialized() else None
        try:
            return fn(self, *args, **kw)
        finally:
            if prev is not None:
                torch.cuda.set_device(prev)
    return wrapper


class _ShardedInfos(LazyInfos):
    """LazyInfos of one MultiDeviceGraphMPEVecEnv step over its shards: `parts` = [(lo, hi, the shard's LazyInfos)]. The first read fills one [N, A, 18] array in
    env order from every shard's rows; a shard whose info buffer a later step has overwritten raises as a single handle's infos do."""

    def __init__(self, parts, n_envs, n_agents, include_min_time, include_phase):
        LazyInfos.__init__(self, None, n_envs, n_agents, include_min_time=include_min_time, include_phase=include_phase)
        self._parts = parts

    def _fetch(self):
        if self._host is None:
            h = np.empty((self._n, self._a, len(INFO_KEYS)))
            for lo, hi, p in self._parts:
                h[lo:hi] = p._fetch()
            self._host, self._parts = h, None
        return self._host


class MultiDeviceGraphMPEVecEnv(object):
    """BatchedGraphMPEVecEnv's surface over several GPUs in ONE process: the drop-in for a runner that stays a single process (train_mpe.py:21-43 has no
    torch.distributed) but should use every GPU of the node.

    Shard g owns the envs sharding.shard_range(N, G, g) on devices[g], as a BatchedGraphMPEVecEnv with env_id_base = lo, so its per-env RNG streams are the
    unsharded run's and every output is bit-identical to one handle over all N envs. Entries of `devices` may repeat: several shards then share a device (that
    rehearses the code path on one GPU; it is not a performance mode). `step_async` queues, device after device, the upload of the shard's slice of the
    actions, the safety filter, the shard's kernel launch and its D2H copies straight into rows [lo, hi) of one pinned [N, ...] host array per output, all on
    the device's current stream; nothing waits until `step_wait`, which synchronises each device and returns views of those arrays. The hand-off rules are
    the single handle's: two alternating sets of host arrays (what step t returned stays valid until step t+2), pinned_host=False returns fresh arrays,
    adj_broadcast_view=True returns the compact E x E matrix as a broadcast view, infos are lazy and double-buffered, sticky device error flags of any shard
    raise GmpeError naming the shard.

    safety_filter: called once per shard and step as f(shard_engine, shard_actions_dev) — it sees one shard at a time: the shard's engine (its cfg has that
    shard's num_envs and env_id_base) and that shard's actions on that shard's device, and returns (ctrl, use) shaped for that shard."""
    closed = False
    viewer = None
    metadata = BatchedGraphMPEVecEnv.metadata

    @_keeps_current_device
    def __init__(self, all_args, devices, num_envs=None, adj_broadcast_view=True, pinned_host=True, safety_filter=None, eval_surface=False):
        self.devices = [int(d) for d in devices]
        self.cfg = config_from_args(all_args, num_envs=num_envs)
        N, G = self.cfg.num_envs, len(self.devices)
        if G == 0:
            raise ValueError("devices must name at least one device")
        if G > N:
            raise ValueError("%d shards for %d envs: every shard needs at least one env" % (G, N))
        self._all_args = all_args
        self._compact, self._pinned, self._eval_surface = bool(adj_broadcast_view), bool(pinned_host), bool(eval_surface)
        self._ranges = [shard_range(N, G, g) for g in range(G)]
        # with pinned_host the shards get two empty sets of host destinations now and their row views of the shared arrays once the output shapes are known
        self._shards = []
        try:
            for d, (lo, hi) in zip(self.devices, self._ranges):
                self._shards.append(self._make_shard(d, num_envs=hi - lo, env_id_base=lo, adj_broadcast_view=self._compact, pinned_host=self._pinned,
                                                     safety_filter=safety_filter, _host=[{}, {}] if self._pinned else None))
        except BaseException:
            for s in self._shards:
                s.engine.close()
            raise
        s0 = self._shards[0]
        self._specs = [(k, tuple(getattr(s0.engine.out, k).shape[1:]), getattr(s0.engine.out, k).dtype) for k in _KEYS[True]]
        self._specs.append(("err", tuple(s0._err_dev.shape[1:]), s0._err_dev.dtype))
        self._host = None
        self._flip = 0
        if self._pinned:
            self._host = [self._host_set() for _ in range(2)]
            for b, h in enumerate(self._host):
                for g, s in enumerate(self._shards):
                    s._host[b].update(self._rows(h, g))
        self.num_envs = N
        self.num_agents = self.n = s0.num_agents
        for k in ("observation_space", "share_observation_space", "action_space", "node_observation_space", "adj_observation_space",
                  "edge_observation_space", "agent_id_observation_space", "share_agent_id_observation_space"):
            setattr(self, k, getattr(s0, k))
        self.waiting = False
        self._pending = None

    @property
    def shard_engines(self):
        """The shards' GmpeEngines in shard (global env) order: engine g steps envs sharding.shard_range(N, G, g) on devices[g]."""
        return [s.engine for s in self._shards]

    def _make_shard(self, device, **kw):
        """One shard: a BatchedGraphMPEVecEnv over envs [env_id_base, env_id_base + num_envs) on `device`."""
        return BatchedGraphMPEVecEnv(self._all_args, device=device, **kw)

    # ------------------------------------------------------------------ helpers
    def _host_set(self):
        """One [N, ...] host tensor per output (and the error flags), allocated like a shard's own."""
        return {k: self._shards[0]._empty_host((self.cfg.num_envs,) + shp, dt, self._pinned) for k, shp, dt in self._specs}

    def _rows(self, h, g):
        lo, hi = self._ranges[g]
        return {k: t[lo:hi] for k, t in h.items()}

    def _queue(self, launch, keys):
        """For every shard in turn: launch(g, shard) -> its outputs, then its D2H copies into its rows of this hand-off's host set. Nothing waits.
        Returns (host set, outputs per shard)."""
        if self._pinned:
            b = self._flip
            self._flip ^= 1
            h = self._host[b]
            dst = [s._host[b] for s in self._shards]
        else:
            h = self._host_set()
            dst = [self._rows(h, g) for g in range(len(self._shards))]
        outs = []
        for g, (s, d) in enumerate(zip(self._shards, dst)):
            o = launch(g, s)
            s._issue(o, keys, d)
            outs.append(o)
        return h, outs

    def _collect(self, h, keys):
        """Wait for every device, raise the shards' sticky errors, -> NumPy views of the host set."""
        for s in self._shards:
            s._sync()
        err = h["err"].numpy()
        msgs = [self._shard_error(g, s._raise_errors) for g, s in enumerate(self._shards) if err[slice(*self._ranges[g])].any()]
        if any(msgs):
            raise _lib.GmpeError("; ".join(m for m in msgs if m))
        arrs = [h[k].numpy() for k in keys]
        arrs[3] = _expand_adj(arrs[3], self.num_agents, self._compact)
        return arrs

    def _shard_error(self, g, check):
        """check() (a shard's error check, or its close) -> None, or the message of the GmpeError it raised, naming shard g."""
        try:
            check()
        except _lib.GmpeError as e:
            lo, hi = self._ranges[g]
            return "shard %d of %d (cuda:%d, envs %d..%d): %s" % (g, len(self._shards), self.devices[g], lo, hi - 1, e)
        return None

    # ------------------------------------------------------------------ GraphSubprocVecEnv surface
    @_keeps_current_device
    def reset(self, num_current_episode=0):
        """-> (obs [N,A,D], agent_id [N,A,1], node_obs [N,A,E,F], adj [N,A,E,E])"""
        h, _ = self._queue(lambda g, s: s.engine.reset(), _KEYS[False])
        return tuple(self._collect(h, _KEYS[False]))

    @_keeps_current_device
    def step_async(self, actions, num_current_episode=None):
        """actions: [N, A, n_actions] one-hot or [N, A] integer indices (NumPy or tensors); shard g gets rows [lo, hi)."""
        if self.waiting:
            raise RuntimeError("step_async called while a step is pending")
        a, kind = _check_actions(actions, self.num_envs, self.num_agents, self.cfg.n_actions)
        self._pending = self._queue(lambda g, s: s._launch(a[slice(*self._ranges[g])], kind), _KEYS[True])
        self.waiting = True

    @_keeps_current_device
    def step_wait(self):
        """-> the 7-tuple of BatchedGraphMPEVecEnv.step_wait over all N envs (8-tuple with eval_surface)."""
        if not self.waiting:
            raise RuntimeError("step_wait without step_async")
        h, outs = self._pending
        self._pending, self.waiting = None, False
        obs, ids, node, adj, rew, done = self._collect(h, _KEYS[True])
        done = done.astype(bool)
        if self.cfg.collaborative:
            rew = rew[..., None]
        infos = _ShardedInfos([(lo, hi, s._infos(o)) for (lo, hi), s, o in zip(self._ranges, self._shards, outs)], self.num_envs, self.num_agents,
                              include_min_time=self.cfg.max_speed > 0, include_phase=self.cfg.scenario in ROT_FAMILY)
        if self._eval_surface:
            reset_count = 1 if done.all(axis=1).any() else 0
            return obs, ids, node, adj, rew, done, infos, reset_count
        return obs, ids, node, adj, rew, done, infos

    step = BatchedGraphMPEVecEnv.step
    reset_task = BatchedGraphMPEVecEnv.reset_task
    render = BatchedGraphMPEVecEnv.render
    seed = BatchedGraphMPEVecEnv.seed
    unwrapped = BatchedGraphMPEVecEnv.unwrapped

    @_keeps_current_device
    def close(self):
        """Closes every shard, also when one of them raises. Sticky device errors no hand-off has raised yet are raised once, naming their shards, after
        every handle is freed (BatchedGraphMPEVecEnv.close's contract, per shard)."""
        if self.closed:
            return
        msgs, other = [], None
        for g, s in enumerate(self._shards):
            try:
                msgs.append(self._shard_error(g, s.close))
            except Exception as e:
                other = other if other is not None else e
        self.closed = True
        if any(msgs):
            raise _lib.GmpeError("; ".join(m for m in msgs if m))
        if other is not None:
            raise other


def _device_arg(device, devices):
    if devices is not None and device is not None:
        raise ValueError("pass device or devices, not both")
    devices = list(devices) if devices is not None else [0 if device is None else device]
    return devices


def make_train_env(all_args, device=None, eval_surface=False, devices=None):
    """Counterpart of onpolicy/scripts/train_mpe.py:21-43 for env_name == 'GraphMPE'. `step` returns the GraphSubprocVecEnv 7-tuple for EVERY thread
    count, one included: that is what the collect / eval loops unpack (graph_mpe_runner.py:83, 490). The reference itself builds GraphDummyVecEnv
    for n_rollout_threads == 1 (train_mpe.py:34-36), whose 8-tuple (env_wrappers.py:920-936) those loops cannot unpack — a single-thread training
    run of the reference raises "too many values to unpack"; only GMPERunner.render wants the 8-tuple (graph_mpe_runner.py:621-622). Pass
    eval_surface=True (or use make_eval_env) to get that shape.
    device: one GPU (default 0). devices: a list of device ordinals — two or more entries spread the envs over them in this process
    (MultiDeviceGraphMPEVecEnv); one entry is `device`. Passing both is a ValueError."""
    if getattr(all_args, "env_name", "GraphMPE") != "GraphMPE":
        raise NotImplementedError("only the GraphMPE route is built")
    devices = _device_arg(device, devices)
    if len(devices) > 1:
        return MultiDeviceGraphMPEVecEnv(all_args, devices, num_envs=all_args.n_rollout_threads, eval_surface=eval_surface)
    return BatchedGraphMPEVecEnv(all_args, num_envs=all_args.n_rollout_threads, device=devices[0], eval_surface=eval_surface)

def GraphMPEEnv(args, device=0):
    """multiagent/MPE_env.py:56-84 builds ONE env; here that is a batch of one."""
    assert "graph" in args.scenario_name, "Only use graph env for graph scenarios"
    return BatchedGraphMPEVecEnv(args, num_envs=1, device=device)



def make_eval_env(all_args, device=None, devices=None):
    """Counterpart of onpolicy/scripts/train_mpe.py:46-68 / eval_mpe.py:21-43: n_eval_rollout_threads == 1 selects GraphDummyVecEnv,
    whose step returns the 8-tuple GMPERunner.render unpacks (graph_mpe_runner.py:621-622). device / devices as in make_train_env."""
    if getattr(all_args, "env_name", "GraphMPE") != "GraphMPE":
        raise NotImplementedError("only the GraphMPE route is built")
    n = getattr(all_args, "n_eval_rollout_threads", 1)
    devices = _device_arg(device, devices)
    if len(devices) > 1:
        return MultiDeviceGraphMPEVecEnv(all_args, devices, num_envs=n, eval_surface=(n == 1))
    return BatchedGraphMPEVecEnv(all_args, num_envs=n, device=devices[0], eval_surface=(n == 1))
