"""DeviceRolloutBuffer — env-side arrays of GraphReplayBuffer kept in HBM.

Mirrors the storage the runner fills from the env (onpolicy/utils/graph_buffer.py:84-164 shapes,
:168-251 insert, :253-283 after_update; masks as computed in
onpolicy/runner/shared/graph_mpe_runner.py:384-428): `[T+1, N, A, ...]` float32/int32 slots for
obs / share_obs / node_obs / adj / agent_id / share_agent_id / masks / active_masks and `[T, N, A, 1]`
rewards. The engine's output pointers are re-bound to slot t+1 before every step, so the kernel writes
the rollout in place: no host hop and no device-to-device copy of the 16 KB/env adjacency.
Opt-in policy-side storage (policy_storage_spec): value_preds / returns / bad_masks / available_actions [T+1, ...] and advantages [T, ...],
with compute_returns / normalized_advantages (GraphReplayBuffer.compute_returns, GR_MAPPO.train's advantage lines) and the stop-action rows of
available_actions (graph_mpe_runner.py:263-335) computed on the device.
Opt-in learner-side storage (learner_storage_spec): rnn_states / rnn_states_critic [T+1, N, A, R, H] and actions / action_log_probs [T, N, A, k], written
with value_preds, the step's masks and its stop rows by ONE launch per step from the policy's outputs (insert_step / insert_external keywords,
gmpe_step_tail: the runner's `rnn_states[dones] = 0` on the device, no host sync) and carried by after_update: with every field kept, the buffer is a whole device GraphReplayBuffer.
act_step puts the action head itself into the step's launch sequence: the policy hands over its logits, one launch (gmpe_act_sample, act.py) masks them from
the previous step's dones, draws the action and writes actions[t] / action_log_probs[t] in place, then the env steps.
The open-loop collect(action_sets) and the sharded collectors (sharding.ShardedRolloutCollector, vec_env.MultiDeviceGraphMPEVecEnv) have no policy output
to store: they never write the learner fields.
"""
import torch

from .config import NODE_FEATS
from .engine import StepOutputs, available_actions_from_dones, compute_returns, denorm_scalars, returns_workspace_bytes, step_tail
from . import _lib
from .minibatch import LEARNER, EdgeList, check_edge_args, edge_list, feed_forward_generator, recurrent_generator

POLICY_FIELDS = ("value_preds", "returns", "bad_masks", "available_actions", "advantages")
LEARNER_FIELDS = ("rnn_states", "rnn_states_critic", "actions", "action_log_probs")


def storage_spec(cfg, episode_length, adj_compact, node_form, with_adj=True):
    """name -> (dtype, shape) of the env-side arrays of a rollout (graph_buffer.py:84-164 shapes). With node_form "table" the node features are kept as the fp64
    entity table [T+1, N, W] they are a pure function of (include/gmpe.h gmpe_outputs.entity_table) instead of the [T+1, N, A, E, F] rows."""
    N, A, E, D = cfg.num_envs, cfg.num_agents, cfg.num_entities, cfg.obs_dim
    T, T1 = int(episode_length), int(episode_length) + 1
    f32 = torch.float32
    spec = {"obs": (f32, (T1, N, A, D))}
    if node_form != "table":
        spec["node_obs"] = (f32, (T1, N, A, E, cfg.node_feats))
    if node_form != "rows":
        spec["entity_table"] = (torch.float64, (T1, N, cfg.entity_table_width))
    if with_adj:
        spec["_adj"] = (f32, (T1, N, E, E) if adj_compact else (T1, N, A, E, E))
    spec["agent_id"] = (torch.int32, (T1, N, A, 1))
    spec["rewards"] = (f32, (T, N, A, 1))
    spec["dones"] = (torch.uint8, (T, N, A))
    spec["masks"] = (f32, (T1, N, A, 1))
    spec["active_masks"] = (f32, (T1, N, A, 1))
    return spec


def policy_storage_spec(cfg, episode_length, fields=POLICY_FIELDS):
    """name -> (dtype, shape) of the policy-side arrays a DeviceRolloutBuffer keeps on request (graph_buffer.py:118-138, 162 shapes; advantages: the
    [T, N, A, 1] array GR_MAPPO.train computes)."""
    N, A = cfg.num_envs, cfg.num_agents
    T, T1 = int(episode_length), int(episode_length) + 1
    shapes = dict(value_preds=(T1, N, A, 1), returns=(T1, N, A, 1), bad_masks=(T1, N, A, 1), available_actions=(T1, N, A, cfg.n_actions),
                  advantages=(T, N, A, 1))
    unknown = set(fields) - set(shapes)
    if unknown:
        raise ValueError("unknown policy fields: %s" % sorted(unknown))
    return {k: (torch.float32, shapes[k]) for k in POLICY_FIELDS if k in fields}


def learner_storage_spec(cfg, episode_length, fields=LEARNER_FIELDS, recurrent_N=1, hidden_size=64, hidden_size_critic=None, act_dim=1):
    """name -> (dtype, shape) of the learner-side arrays a DeviceRolloutBuffer keeps on request (graph_buffer.py:114-120, 142-154 shapes, float32, zeros):
    rnn_states [T+1, N, A, recurrent_N, hidden_size], rnn_states_critic the same with hidden_size_critic (default hidden_size, as the reference's
    zeros_like), actions / action_log_probs [T, N, A, act_dim] (1 for the discrete action space)."""
    N, A = cfg.num_envs, cfg.num_agents
    T, T1 = int(episode_length), int(episode_length) + 1
    R, H, k = int(recurrent_N), int(hidden_size), int(act_dim)
    Hc = H if hidden_size_critic is None else int(hidden_size_critic)
    if min(R, H, Hc, k) < 1:
        raise ValueError("recurrent_N, hidden_size, hidden_size_critic and act_dim must be >= 1")
    shapes = dict(rnn_states=(T1, N, A, R, H), rnn_states_critic=(T1, N, A, R, Hc), actions=(T, N, A, k), action_log_probs=(T, N, A, k))
    unknown = set(fields) - set(shapes)
    if unknown:
        raise ValueError("unknown learner fields: %s" % sorted(unknown))
    return {k_: (torch.float32, shapes[k_]) for k_ in LEARNER_FIELDS if k_ in fields}


_ONES = ("masks", "active_masks", "bad_masks", "available_actions")   # what GraphReplayBuffer starts with ones (graph_buffer.py:132, 155-162)


class DeviceRolloutBuffer(object):
    def __init__(self, engine, episode_length, use_centralized_V=True, storage=None, policy_fields=None, args=None, learner_fields=None,
                 recurrent_N=None, hidden_size=None, hidden_size_critic=None, act_dim=None):
        """storage: optional dict name -> caller-owned tensor for some or all of the arrays of storage_spec (e.g. views of ONE byte slab that a collective ships
        as a whole, sharding.ShardedRolloutCollector); anything missing is allocated here.
        policy_fields: None (none), "all", or some of POLICY_FIELDS — the policy-side arrays of policy_storage_spec this buffer keeps (a storage entry of
        such a name requests it too). args: the runner's args (gamma, gae_lambda, use_gae, use_proper_time_limits, use_valuenorm, use_popart), read by
        compute_returns / normalized_advantages.
        learner_fields: None (none), "all", or some of LEARNER_FIELDS — the learner-side arrays of learner_storage_spec this buffer keeps (a storage entry
        of such a name requests it too), written by insert_step / insert_external from the policy's outputs. Their sizes: recurrent_N / hidden_size from
        these keywords, else from args, else the reference's defaults (1, 64); hidden_size_critic defaults to hidden_size, act_dim to 1 (Discrete)."""
        self.engine = engine
        self.T = int(episode_length)
        self.use_centralized_V = bool(use_centralized_V)
        c, dev = engine.cfg, engine.device
        self.node_form, self.adj_form = engine.node_form, engine.adj_form
        self.args = args
        storage = dict(storage or {})
        policy = set(POLICY_FIELDS if policy_fields == "all" else (policy_fields or ())) | (set(storage) & set(POLICY_FIELDS))
        spec = storage_spec(c, self.T, engine.adj_compact, self.node_form, with_adj=self.adj_form != "none")
        spec.update(policy_storage_spec(c, self.T, policy))
        learner = set(LEARNER_FIELDS if learner_fields == "all" else (learner_fields or ())) | (set(storage) & set(LEARNER_FIELDS))
        pick = lambda v, name, default: int(v) if v is not None else int(getattr(args, name, default) if args is not None else default)
        spec.update(learner_storage_spec(c, self.T, learner, recurrent_N=pick(recurrent_N, "recurrent_N", 1), hidden_size=pick(hidden_size, "hidden_size", 64),
                                         hidden_size_critic=hidden_size_critic, act_dim=1 if act_dim is None else act_dim))
        self._adj = None
        for name in POLICY_FIELDS + LEARNER_FIELDS:
            setattr(self, name, None)
        for name, (dt, shape) in spec.items():
            t = storage.pop(name, None)
            if t is None:
                t = (torch.ones if name in _ONES else torch.zeros)(shape, dtype=dt, device=dev)
            elif tuple(t.shape) != tuple(shape) or t.dtype != dt or t.device != dev or not t.is_contiguous():
                raise ValueError("storage[%r] must be a contiguous %s tensor of shape %s on %s" % (name, dt, tuple(shape), dev))
            elif name in _ONES:
                t.fill_(1.0)
            setattr(self, name if name != "node_obs" else "_node_obs", t)
        if storage:
            raise ValueError("unknown storage entries: %s" % sorted(storage))
        self._ws = torch.empty((returns_workspace_bytes(c.num_envs * c.num_agents),), dtype=torch.uint8, device=dev) if self.advantages is not None else None
        if self.node_form == "table":
            self._node_obs = None
        if self.node_form == "rows":
            self.entity_table = None
        self.info = torch.zeros_like(engine.out.info) if engine.out.info is not None else None
        self.step = 0
        tu = engine.tuning()                                     # fixed by gmpe_create
        self._one_launch = bool(tu["roll"]) and not tu["split"]
        self._prepared = {}

    @property
    def node_obs(self):
        """[T+1, N, A, E, F]. With node_form "table" the rows are expanded from the entity tables on demand (gmpe_expand_node_obs: bit-identical to the rows the engine
        would have written) — a fresh tensor every call; a learner keeps the result, a rank that only ships its rollout never asks."""
        if self._node_obs is not None:
            return self._node_obs
        return self.engine.expand_node_obs(self.entity_table)

    # ------------------------------------------------------------------ views with the reference's shapes
    @property
    def adj(self):
        """[T+1, N, A, E, E]; a zero-copy broadcast when the engine writes the compact matrix; rebuilt from the entity tables (gmpe_expand_adj, bit-identical) when
        the engine writes no adjacency at all (adj_form 'none')."""
        if self._adj is None:
            a = self.engine.expand_adj(self.entity_table)
            T1, N, E, _ = a.shape
            return a[:, :, None].expand(T1, N, self.engine.A, E, E)
        if self.engine.adj_compact:
            T1, N, E, _ = self._adj.shape
            return self._adj[:, :, None].expand(T1, N, self.engine.A, E, E)
        return self._adj

    @property
    def share_obs(self):
        """graph_mpe_runner.py:408-413: every agent sees the concatenation of all agents' obs."""
        T1, N, A, D = self.obs.shape
        if not self.use_centralized_V:
            return self.obs
        return self.obs.reshape(T1, N, 1, A * D).expand(T1, N, A, A * D)

    @property
    def share_agent_id(self):
        T1, N, A, _ = self.agent_id.shape
        if not self.use_centralized_V:
            return self.agent_id
        return self.agent_id.reshape(T1, N, 1, A).expand(T1, N, A, A)

    # ------------------------------------------------------------------ filling
    def _slot(self, t):
        """Slot t of the arrays as engine outputs — reward / done of slot t - 1, the step that writes slot t; the engine's own buffers at t = 0, where a reset
        writes none — and the elements between consecutive slots of every array (the rollout kernel's strides; info is one buffer every step overwrites)."""
        e = self.engine
        arrays = dict(obs=self.obs, agent_id=self.agent_id, node_obs=self._node_obs, entity_table=self.entity_table, adj=self._adj)
        lagged = dict(reward=self.rewards.view(self.T, e.N, e.A), done=self.dones)
        o = {k: None if v is None else v[t] for k, v in arrays.items()}
        o.update({k: v[t - 1] for k, v in lagged.items()} if t else dict(reward=e.out.reward, done=e.out.done))
        strides = {k: v.numel() // v.shape[0] for k, v in dict(arrays, **lagged).items() if v is not None}
        strides["masks"] = e.N * e.A
        return StepOutputs(info=self.info, **o), strides

    def _bind(self, t):
        self.engine.rebind(self._slot(t)[0])

    def warmup(self):
        """GMPERunner.warmup (graph_mpe_runner.py:213-238): reset outputs go to slot 0."""
        self._bind(0)
        self.engine.reset()
        self.step = 0

    def insert_step(self, action_idx, values=None, *, actions=None, action_log_probs=None, rnn_states=None, rnn_states_critic=None):
        """One env step written straight into slot step+1 (+ masks), GraphReplayBuffer.insert semantics. `values` (the policy's [N, A, 1] values of this
        step, buffer with value_preds) go to value_preds[step] (graph_buffer.py:234); with available_actions the step's stop-action slot is written too.
        The learner keywords take the policy's own outputs of this step in its [N*A, ...] shapes — actions int64 [N*A, k], action_log_probs [N*A, k],
        rnn_states / rnn_states_critic [N*A, R, H] — each needing its buffer array (learner_fields). With any of them the env step runs first, then ONE launch
        (gmpe_step_tail) writes values, actions[step], action_log_probs[step] and the RNN states of slot step + 1 with the rows of the agents this
        step made done zeroed (GMPERunner.insert, graph_mpe_runner.py:386-392), and with them the masks and the step's stop-action slot."""
        t = self.step
        learner = self._learner_inputs(values, actions, action_log_probs, rnn_states, rnn_states_critic, "insert_step")
        if learner is not None:
            self._bind(t + 1)
            self.engine.step(action_idx)
            self._step_tail(t, learner)
            self.step = (t + 1) % self.T
            return self.engine.out
        if values is not None:
            if self.value_preds is None:
                raise ValueError("insert_step(values=...) needs a buffer with value_preds (policy_fields)")
            self.value_preds[t].copy_(torch.as_tensor(values).reshape(self.value_preds[t].shape))
        self.available_actions_for(t)
        self._bind(t + 1)
        self.engine.step(action_idx)
        # masks[dones] = 0; active_masks[dones] = 0 except where the whole env is done — one small kernel instead of eight torch ops
        self.engine.masks_from_dones(self.dones[t], self.masks[t + 1], self.active_masks[t + 1])
        self.step = (t + 1) % self.T
        return self.engine.out

    act_draw = 0            # the call counter of act_step's action stream: one value per act, carried by carry_from
    _act_idx = _act_logp = _act_draw_dev = None
    _tail_draw_dev = None   # set by gmpe.policy.collect_step for one act_finish: the counter its sampling launch read and left for the tail to advance

    def _step_tail(self, t, learner, draw_dev=None):
        """What follows the env step of step t, one launch (engine.step_tail, gmpe_step_tail): masks[t + 1] / active_masks[t + 1], the stop rows of
        available_actions[t + 1] where the buffer keeps them — what available_actions_for(t) writes, which nothing reads before the step ends —, the
        learner fields of `learner` (_learner_inputs' dict, or None) and, with draw_dev, the draw counter's advance by one."""
        step_tail(t, self.dones, self._learner_arrays(), num_agents=self.engine.A, masks=self.masks, active_masks=self.active_masks,
                  available_actions=self.available_actions, draw_dev=draw_dev, draw_inc=0 if draw_dev is None else 1, **(learner or {}))

    def act_draw_counter(self):
        """act_draw as an int64 [1] device tensor, created on demand: what the steps of a captured rollout hand the sampling launch as draw_dev
        (gmpe.policy.CapturedRollout), which advances it by one per step on the stream. The host's act_draw stays the truth: whoever launches such steps
        first makes the counter equal to it (sync_act_draw_counter) and afterwards adds the steps to act_draw."""
        if self._act_draw_dev is None:
            self._act_draw_dev = torch.full((1,), int(self.act_draw), dtype=torch.int64, device=self.engine.device)
        return self._act_draw_dev

    def sync_act_draw_counter(self):
        """counter = act_draw, one fill on the current stream (nothing where no counter was asked for); nothing waits for the device"""
        if self._act_draw_dev is not None:
            self._act_draw_dev.fill_(int(self.act_draw))

    def act_step(self, logits, values=None, *, rnn_states=None, rnn_states_critic=None, deterministic=False):
        """insert_step with the action head in the launch sequence: `logits` (the policy head's linear output of this step, [N*A, n_actions], before
        masking) instead of an action. One launch (gmpe_act_sample, act.sample_actions) masks them with the availability of this step — taken from
        dones[step - 1] directly, all available at step 0; the available_actions slot is still written, after the env step, when the buffer keeps that
        field —, draws the action (or takes the mode with deterministic=True) and writes actions[step] and action_log_probs[step] into their slots in
        place (when the buffer keeps them) and the int32 action into a tensor the buffer owns; then the env step and one gmpe_step_tail launch for the
        masks, the stop rows and whatever else was given (values, rnn_states, rnn_states_critic, as insert_step's). The draw of a row is keyed by the engine's seed, the env's
        global id (cfg.env_id_base), the agent and `act_draw`, which advances by one per call: the same envs take the same actions however they are
        spread over buffers. The stored log-probs are bit for bit what ppo_losses recomputes from the same logits."""
        from .act import sample_actions
        t, e = self.step, self.engine
        c, rows = e.cfg, e.N * e.A
        learner = self._learner_inputs(values, None, None, rnn_states, rnn_states_critic, "act_step")
        if not isinstance(logits, torch.Tensor) or logits.dim() != 2 or tuple(logits.shape) != (rows, c.n_actions):
            raise ValueError("logits must be a tensor of shape (%d, %d)" % (rows, c.n_actions))
        out = self.act_outputs()
        sample_actions(logits, dones_prev=self.dones[t - 1] if t else None, stop_action=c.n_actions // 2 if t else None, seed=c.seed,
                       env_id_base=c.env_id_base, num_agents=e.A, draw=self.act_draw, deterministic=deterministic, out=out)
        return self.act_finish(learner)

    def act_outputs(self):
        """The `out` of the sampling launch of step `self.step` (act.sample_actions, head.act_head): actions[step] and action_log_probs[step] in place
        where the buffer keeps them, the log-probs else into scratch the buffer owns, and the int32 action the env step then reads. What act_step
        hands its own launch; gmpe.policy.collect_step hands it to the actor's."""
        t, e = self.step, self.engine
        out = {}
        for name, key in (("actions", "actions_f32"), ("action_log_probs", "action_log_probs")):
            buf = getattr(self, name)
            if buf is not None:
                if buf.shape[-1] != 1:
                    raise NotImplementedError("%s of shape %s: only a single Discrete head is supported (MultiDiscrete, mixed and continuous heads "
                                              "are not)" % (name, tuple(buf.shape)))
                out[key] = buf[t]
        if self._act_idx is None:
            self._act_idx = torch.zeros((e.N, e.A), dtype=torch.int32, device=e.device)
        if "action_log_probs" not in out:
            if self._act_logp is None:
                self._act_logp = torch.zeros((e.N * e.A, 1), dtype=torch.float32, device=e.device)
            out["action_log_probs"] = self._act_logp
        out["action_idx"] = self._act_idx
        return out

    def act_finish(self, learner=None):
        """What follows the sampling launch of step `self.step`: the env step on the action act_outputs() received, one gmpe_step_tail launch for the
        masks, the step's stop rows and `learner` (_learner_inputs' dict, or None) — and for the device draw counter, where collect_step left one in
        _tail_draw_dev —, and the two host counters."""
        t, e = self.step, self.engine
        draw_dev, self._tail_draw_dev = self._tail_draw_dev, None
        self._bind(t + 1)
        e.step(self._act_idx)
        self._step_tail(t, learner, draw_dev)
        self.act_draw += 1
        self.step = (t + 1) % self.T
        return e.out

    def insert_external(self, obs, agent_id, node_obs, adj, rewards, dones, values=None, *, actions=None, action_log_probs=None, rnn_states=None,
                        rnn_states_critic=None):
        """GraphReplayBuffer.insert's env-side arguments for step outputs produced elsewhere (a replayed log, another engine):
        device or host tensors in the engine's shapes ([N,A,D], [N,A,1], [N,A,E,F], [N,E,E] or [N,A,E,E], [N,A], [N,A] bool/u8).
        Same slot placement and mask rules as insert_step (graph_buffer.py:223-251, graph_mpe_runner.py:395-405); the policy keywords as insert_step's,
        written with the masks and the stop rows by one launch after the dones."""
        t, e = self.step, self.engine
        learner = self._learner_inputs(values, actions, action_log_probs, rnn_states, rnn_states_critic, "insert_external")
        dev = e.device
        put = lambda dst, src: dst.copy_(torch.as_tensor(src).to(device=dev, dtype=dst.dtype).reshape(dst.shape))
        if self._node_obs is None:
            raise ValueError("insert_external takes node_obs rows: the buffer's engine must keep them (node_form 'rows' or 'both')")
        put(self.obs[t + 1], obs); put(self.agent_id[t + 1], agent_id); put(self._node_obs[t + 1], node_obs)
        if self._adj is None:
            raise ValueError("insert_external takes an adjacency: the buffer's engine must keep one (adj_form not 'none')")
        a = torch.as_tensor(adj)
        if e.adj_compact and a.dim() == 4:
            a = a[:, 0]                                   # the A per-agent matrices are one matrix (…_july.py:1625)
        elif not e.adj_compact and a.dim() == 3:
            a = a[:, None].expand(-1, e.A, -1, -1)
        put(self._adj[t + 1], a); put(self.rewards[t], rewards); put(self.dones[t], torch.as_tensor(dones).to(torch.uint8))
        self._step_tail(t, learner)
        self.step = (t + 1) % self.T

    def _learner_arrays(self):
        return {k: getattr(self, k) for k in ("value_preds",) + LEARNER_FIELDS if getattr(self, k) is not None}

    def _learner_inputs(self, values, actions, action_log_probs, rnn_states, rnn_states_critic, what):
        """The policy's outputs as device tensors for step_tail (no copy when they already are: float32, int64 actions kept), or None when only
        `values` (or nothing) is given to insert_step, which keeps its own path. A field the buffer does not keep raises ValueError."""
        given = dict(values=values, actions=actions, action_log_probs=action_log_probs, rnn_states=rnn_states, rnn_states_critic=rnn_states_critic)
        if all(given[k] is None for k in LEARNER_FIELDS) and (what == "insert_step" or values is None):
            return None
        dev = self.engine.device
        out = {}
        for name, x in given.items():
            if x is None:
                continue
            dst = "value_preds" if name == "values" else name
            if getattr(self, dst) is None:
                raise ValueError("%s(%s=...) needs a buffer with %s (%s)" % (what, name, dst, "policy_fields" if name == "values" else "learner_fields"))
            x = torch.as_tensor(x).to(device=dev)
            if not (name == "actions" and x.dtype == torch.int64):
                x = x.to(torch.float32)
            out[name] = x.contiguous()
        return out

    def collect(self, action_sets, num_steps=None):
        """The runner's collect loop with a fixed action source (graph_mpe_runner.py:57-103: `for step in range(episode_length)`:
        envs.step -> buffer.insert) as ONE launch of the persistent rollout kernel: step k reads action_sets[k % S] and writes slot
        step+k+1 of every array in place, masks / active_masks included (gmpe_rollout_steps). Same results as `num_steps`
        insert_step calls. Falls back to that loop on the split big-E path. There is no policy output here: the learner fields are not written."""
        K = self.T - self.step if num_steps is None else int(num_steps)
        e, a = self.engine, action_sets
        if not self._one_launch:
            for k in range(K):
                self.insert_step(a[k % a.shape[0]])
            return e.out
        # the same rollout as an earlier call: one C call, no views / structs rebuilt (engine.prepare_rollout). Another view of the same address is another key,
        # prepared (and checked) again.
        key = (a.data_ptr(), a.device, a.dtype, a.shape, a.stride(), K, self.step)
        hit = self._prepared.get(key)
        if hit is None:
            slot0, strides = self._slot(1)
            launch = e.prepare_rollout(a, K, slot0=slot0, num_slots=self.T, first_slot=self.step, strides=strides,
                                       masks=self.masks[1], active_masks=self.active_masks[1])
            if len(self._prepared) >= 8:
                self._prepared.clear()
            hit = self._prepared[key] = (launch, a)             # keeps the action tensor alive: its address is part of the key
        hit[0]()
        if self.available_actions is not None:                  # the K steps' stop-action slots from the dones just written: one more launch
            available_actions_from_dones(self.dones, self.available_actions[1:], first=self.step, count=K)
        # the engine's "current outputs" are the last slot written, as after insert_step
        self._bind((self.step + K - 1) % self.T + 1)
        self.step = (self.step + K) % self.T
        return e.out

    def after_update(self):
        """graph_buffer.py:253-283: the last slot becomes slot 0 of the next rollout (rnn_states / rnn_states_critic included; actions and
        action_log_probs have no slot T)."""
        for buf in self._carried():
            buf[0].copy_(buf[-1])

    def _carried(self):
        return [b for b in (self.obs, self._node_obs, self.entity_table, self._adj, self.agent_id, self.masks, self.active_masks,
                            self.bad_masks, self.available_actions, self.rnn_states, self.rnn_states_critic) if b is not None]

    def _arrays(self):
        """(name, tensor) of every device tensor the buffer holds as an attribute, by name: the arrays, the returns workspace, info, the action scratch
        and the draw counter. Whoever must save, restore or guard all of a buffer's storage (gmpe.policy.CapturedRollout) asks here, so that an
        array added later is included without being listed anywhere else."""
        return [(k, v) for k, v in sorted(vars(self).items()) if isinstance(v, torch.Tensor)]

    # ------------------------------------------------------------------ policy side (opt-in: policy_fields)
    def available_actions_for(self, step):
        """The [N, A, n_actions] availability the policy acts with at `step` (graph_mpe_runner.py:73-141: all ones at step 0, else collect_with_mask's
        stop rows from the dones of step - 1), written into its buffer slot step + 1 (graph_buffer.py:249-250) by one small launch and returned as a view.
        None when the buffer keeps no available_actions."""
        if self.available_actions is None:
            return None
        available_actions_from_dones(self.dones, self.available_actions[1:], first=int(step), count=1)
        return self.available_actions[int(step) + 1]

    def _flags(self, what):
        a = self.args
        if a is None:
            raise ValueError("%s needs the runner's args (DeviceRolloutBuffer(..., args=...))" % what)
        return a, bool(getattr(a, "use_popart", False) or getattr(a, "use_valuenorm", False))

    def _denorm(self, use_norm, value_normalizer, what):
        if not use_norm:
            return None
        if value_normalizer is None:
            raise ValueError("%s: args.use_valuenorm / use_popart is set, so a value_normalizer is required" % what)
        return denorm_scalars(value_normalizer, self.engine.device)

    def compute_returns(self, next_value, value_normalizer=None, shards=None):
        """GraphReplayBuffer.compute_returns (graph_buffer.py:285-366) with the runner's args, one launch on the current stream: returns[0..T-1], the
        reference's side effect (value_preds[T] = next_value with use_gae, returns[T] = next_value without), and — buffer with advantages — the raw
        advantages returns[t] - denorm(value_preds[t]). next_value: [N, A, 1] values of the last slot (graph_mpe_runner.py:431-443).
        shards: the exchange of a data-parallel learner (gmpe.learner_shards) or None. Returns and raw advantages are lane-local, so this call
        reduces over nothing and exchanges nothing: a rank's result is the unsharded one on its lanes either way; the argument is checked and
        accepted so that the learner passes the same `shards` along its whole path (normalized_advantages is where it acts)."""
        if shards is not None:
            from .learner_shards import check_shards
            check_shards(shards)
        if self.value_preds is None or self.returns is None:
            raise ValueError("compute_returns needs a buffer with value_preds and returns (policy_fields)")
        a, use_norm = self._flags("compute_returns")
        proper = bool(getattr(a, "use_proper_time_limits", False))
        if proper and self.bad_masks is None:
            raise ValueError("use_proper_time_limits needs a buffer with bad_masks (policy_fields)")
        nv = torch.as_tensor(next_value).to(device=self.engine.device, dtype=torch.float32).contiguous()
        compute_returns(self.rewards, self.masks, self.value_preds, self.returns, nv, gamma=a.gamma, gae_lambda=a.gae_lambda, use_gae=bool(a.use_gae),
                        use_proper_time_limits=proper, bad_masks=self.bad_masks, denorm=self._denorm(use_norm, value_normalizer, "compute_returns"),
                        advantages=self.advantages)
        return self.returns

    def normalized_advantages(self, value_normalizer=None, shards=None):
        """The head of GR_MAPPO.train (graph_mappo.py:294-304): advantages = returns[:-1] - denorm(value_preds[:-1]), normalised by the mean / population
        std of the entries with active_masks[:-1] != 0: (adv - mean) / (std + 1e-5), written into the buffer's advantages (three launches, no host sync).
        shards: the exchange of a data-parallel learner (gmpe.learner_shards) or None: the mean / std are then those over the buffers of ALL ranks, the
        same bits on every rank (four launches around shards.exchange)."""
        if self.advantages is None or self.value_preds is None or self.returns is None:
            raise ValueError("normalized_advantages needs a buffer with value_preds, returns and advantages (policy_fields)")
        _, use_norm = self._flags("normalized_advantages")
        compute_returns(None, None, self.value_preds, self.returns, advantages_only=True, denorm=self._denorm(use_norm, value_normalizer, "normalized_advantages"),
                        advantages=self.advantages, normalized=self.advantages, active_masks=self.active_masks, workspace=self._ws, shards=shards)
        return self.advantages

    # ------------------------------------------------------------------ PPO minibatches (GraphReplayBuffer's generators, gmpe_minibatch_gather)
    def minibatch_arrays(self, learner=None, table=False):
        """The arrays a minibatch gathers from, in the storage form the buffer keeps (node rows or entity table; materialised, compact or no adjacency) plus the
        learner arrays (rnn_states / rnn_states_critic [T+1, N, A, R, H], actions / action_log_probs [T, N, A, k]): the buffer's own (learner_fields), each
        overridden by an array of the same name in `learner`. table: the entity table too wherever the buffer keeps one (adj="table" addresses a minibatch
        through it, whatever else is kept)."""
        e = self.engine
        N, A, T1 = e.N, e.A, self.T + 1
        arrays = dict(obs=self.obs, agent_id=self.agent_id, masks=self.masks, active_masks=self.active_masks, value_preds=self.value_preds,
                      returns=self.returns, available_actions=self.available_actions)
        if self._node_obs is not None:
            arrays["node_obs"] = self._node_obs
        else:
            arrays["entity_table"] = self.entity_table
        if self._adj is not None:
            arrays["adj"] = self._adj
        elif self.entity_table is not None:
            arrays["entity_table"] = self.entity_table
        if table and self.entity_table is not None:
            arrays["entity_table"] = self.entity_table
        for name in LEARNER_FIELDS:
            if getattr(self, name, None) is not None:
                arrays[name] = getattr(self, name)
        learner = dict(learner or {})
        unknown = set(learner) - set(LEARNER)
        if unknown:
            raise ValueError("unknown learner arrays: %s (expected some of %s)" % (sorted(unknown), list(LEARNER)))
        for name, t in learner.items():
            lead, nd = ((T1, N, A), 5) if name.startswith("rnn") else ((self.T, N, A), 4)
            if not isinstance(t, torch.Tensor) or t.dim() != nd or tuple(t.shape[:3]) != lead:
                raise ValueError("learner[%r] must be a tensor of shape %s + %s" % (name, lead, "(R, H)" if nd == 5 else "(k,)"))
        arrays.update(learner)
        return arrays

    def _advantages(self, advantages):
        if advantages is None:
            return None
        t = torch.as_tensor(advantages)
        if tuple(t.shape) != (self.T, self.engine.N, self.engine.A, 1):
            raise ValueError("advantages must have shape %s" % ((self.T, self.engine.N, self.engine.A, 1),))
        return t.to(device=self.engine.device, dtype=torch.float32).contiguous()

    def feed_forward_generator(self, advantages, num_mini_batch=None, mini_batch_size=None, *, learner=None, perm=None, adj="matrix", max_edge_dist=None,
                               inclusive=False):
        """GraphReplayBuffer.feed_forward_generator (graph_buffer.py:368-465) from the device arrays: the reference's 16-tuple per minibatch as fresh device
        tensors (agent_id / share_agent_id int32; available_actions None when the buffer keeps none, learner slots None
        unless the buffer or `learner` holds them), one gather launch per minibatch (two with the entity-table forms). perm: None draws torch.randperm on the CPU default
        generator as the reference does (a seeded run trains on the same minibatches) and uploads it once; "device" draws on the device; or an int64 tensor.
        adj="edges" (with max_edge_dist, inclusive): entry 3 is the minibatch's EdgeList — process_adj's result, computed once for actor and critic from the
        adjacency form the buffer stores (gmpe_minibatch_edges) — and no [rows, E, E] batch is written.
        adj="table" (a buffer that keeps entity tables: node_form "table" or "both"): entry 2 is None and entry 3 the minibatch's gmpe.minibatch.TableRows —
        this buffer's entity_table, not copied, and one int64 per row — for gmpe.gnn_base_from_table; neither the rows nor the matrices are written."""
        check_edge_args(adj, max_edge_dist)
        return feed_forward_generator(self.engine.cfg, self.minibatch_arrays(learner, adj == "table"), self._advantages(advantages), num_mini_batch, mini_batch_size,
                                      perm=perm, use_centralized_V=self.use_centralized_V, adj=adj, max_edge_dist=max_edge_dist, inclusive=inclusive)

    def recurrent_generator(self, advantages, num_mini_batch, data_chunk_length, *, learner=None, perm=None, adj="matrix", max_edge_dist=None, inclusive=False):
        """GraphReplayBuffer.recurrent_generator (graph_buffer.py:599-758): chunks of data_chunk_length samples in the reference's [N, A, T] order, rows
        l * chunks + k, rnn states [chunks, R, H] from each chunk's first sample. perm as feed_forward_generator (over the T*N*A // L chunks); adj,
        max_edge_dist, inclusive as feed_forward_generator."""
        check_edge_args(adj, max_edge_dist)
        return recurrent_generator(self.engine.cfg, self.minibatch_arrays(learner, adj == "table"), self._advantages(advantages), num_mini_batch, data_chunk_length,
                                   perm=perm, use_centralized_V=self.use_centralized_V, adj=adj, max_edge_dist=max_edge_dist, inclusive=inclusive)

    def step_edges(self, step, max_edge_dist, inclusive=False, index64=True, cap=None):
        """process_adj's edge list of slot `step` for the closed loop (the [N*A, E, E] batch the runner feeds the policy), from whichever adjacency form the
        buffer stores -> EdgeList. The compact matrix goes through gmpe_edges_from_adj_compact (each matrix read once for its A copies); the materialised
        matrices and the table-only form (adj_form "none") through gmpe_minibatch_edges with the identity permutation. All give the same result."""
        check_edge_args("edges", max_edge_dist, cap)
        step = int(step)
        if not 0 <= step <= self.T:
            raise ValueError("step must lie in [0, %d]" % self.T)
        e = self.engine
        E = e.cfg.num_entities
        if self._adj is not None and self._adj.dim() == 4:
            ei, ea, m = e.edges_from_adj_compact(self._adj[step], e.A, max_edge_dist, inclusive=inclusive, cap=cap, index64=index64)
            return EdgeList(ei, ea.view(-1, 1), e.N * e.A, E, m)
        if self._adj is not None:
            source, src = _lib.MBE_ADJ, self._adj
        elif self.entity_table is not None:
            source, src = _lib.MBE_TABLE, self.entity_table
        else:
            raise ValueError("the buffer stores no adjacency form (neither adj nor the entity table)")
        out = edge_list(e.cfg, e.device, source, src[step:], 1, e.N, e.A, E, max_edge_dist, perm=None, offset=0, rows=e.N * e.A, inclusive=inclusive,
                        index64=index64, cap=cap)
        if cap is None:
            return out
        m = int(out.n_edges.item())                          # as edges_from_adj_compact: the count on the host, the outputs cut to it
        return EdgeList(out.edge_index[:, :min(m, cap)], out.edge_attr[:min(m, cap)], out.num_graphs, E, m)

    def naive_recurrent_generator(self, advantages, num_mini_batch):
        raise NotImplementedError(
            "naive_recurrent_generator is not provided: the reference's version cannot run for any batch larger than 1 — it flattens masks to [T*N*A, 1] "
            "(graph_buffer.py:501) and then indexes masks[:-1, ind] (:541), which raises IndexError. Use recurrent_generator or feed_forward_generator.")

    def carry_from(self, other):
        """after_update across TWO buffers that alternate (sharding.ShardedRolloutCollector): slot 0 of this one = the last slot of `other`, and the engine's
        outputs are re-bound to this buffer's storage by the next collect / insert_step."""
        for dst, src in zip(self._carried(), other._carried()):
            dst[0].copy_(src[-1])
        self.act_draw = other.act_draw
        self.sync_act_draw_counter()
        self.step = 0
