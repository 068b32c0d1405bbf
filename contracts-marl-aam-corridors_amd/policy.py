"""The reference's actor and critic composed from the device layers: composition only, no arithmetic of its own.

    GR_Actor.forward      ->  actor_forward(actor, ...)    = gnn_base -> mlp_base((obs, nbd)) -> rnn_layer -> act_head
    GR_Critic.forward     ->  critic_forward(critic, ...)  = gnn_base -> mlp_base((cent_obs, nbd)) -> rnn_layer -> F.linear(v_out)
    GR_MAPPOPolicy.get_actions / get_values               ->  get_actions(actor, critic, ...) / get_values(critic, ...): the critic chain ends in value_head
    GMPERunner.collect / collect_with_mask + insert       ->  collect_step(actor, critic, buffer)
    GMPERunner.compute                                    ->  compute(critic, buffer, value_normalizer)
    run()'s loop over one episode, and one whole iteration  ->  rollout(actor, critic, buffer, ...), iteration(actor, critic, ..., buffer, args, ...)
    GMPERunner.eval                                       ->  eval_episode(actor, eval_engine, args)
    GMPERunner.run                                        ->  run(actor, critic, actor_optimizer, critic_optimizer, buffer, args, ..., on_log=, on_eval=, on_save=)
    evaluate_actions + the loss arithmetic of ppo_update  ->  minibatch_losses(actor, critic, sample, args, ...)
    GR_MAPPO.ppo_update                                   ->  ppo_update(actor, critic, actor_optimizer, critic_optimizer, sample, args, ...)
    GR_MAPPO.train                                        ->  train(actor, critic, actor_optimizer, critic_optimizer, buffer, args, ...)
    one update / one episode's rollout as a replayed graph ->  CapturedUpdate(...).update / .train, CapturedRollout(...).replay; run(..., captured=True)
    the evaluator's act callable                          ->  evaluator_act(actor, evaluator)

The modules are the caller's unchanged GR_Actor / GR_Critic (onpolicy/algorithms/graph_actor_critic.py), read by their attribute names (.gnn_base, .base,
.rnn, .act, .v_out, .args); the parameters stay where they are, so the optimisers and the checkpoints do not change. Everything a layer refuses is
refused here by that layer, in its words. In a rollout v_out is value_head, the dot product ppo_losses_popart evaluates in training with --use_popart, so
the stored value_preds are what that loss recomputes; critic_forward and, by default, the learner entries keep torch's F.linear on the caller's weight
and bias for a plain nn.Linear v_out (value_head="device" takes value_head there too). There is no torch fallback: the arrays must be on a HIP device.
"""
import collections

import torch
import torch.nn.functional as F

from .gnn import MAX_NODES as GNN_MAX_NODES, gnn_base, gnn_base_from_table, gnn_base_wide, gnn_base_wide_from_table
from .gru import rnn_layer
from .head import act_head, action_logits
from .minibatch import TableRows
from .mlp import mlp_base
from . import infos as _infos
from . import optim as _optim
from .optim import clip_and_step
from .ppo_loss import ppo_losses, ppo_losses_popart
from . import value as _value


def _recurrent(net):
    """whether the module runs its RNNLayer: the reference's two flags where it has them, else whether there is an .rnn"""
    if hasattr(net, "_use_recurrent_policy") or hasattr(net, "_use_naive_recurrent_policy"):
        return bool(getattr(net, "_use_recurrent_policy", False) or getattr(net, "_use_naive_recurrent_policy", False))
    return getattr(net, "rnn", None) is not None


def _features(net, own_obs, node_obs, adj, agent_id, rnn_states, masks):
    """(features [rows, 64], rnn_states) of an actor or a critic in front of its head; own_obs None: the graph features alone enter the MLPBase.
    adj a gmpe.minibatch.TableRows (node_obs is then not read): the GNNBase runs straight from the entity table, graph r the view of ego agent_id[r] of
    table row index[r] — or, without an index, of row r // num_agents: a rollout step's [N, W] table. Graphs of more than 64 nodes (up to 128) go to the
    forward-only gnn_base_wide / gnn_base_wide_from_table, which refuse a call that needs gradients by name: rollout and evaluation run there, training
    does not."""
    if isinstance(adj, TableRows):
        share = None if adj.index is not None else int(adj.cfg.num_agents)
        table = gnn_base_wide_from_table if int(adj.cfg.num_entities) > GNN_MAX_NODES else gnn_base_from_table
        nbd = table(adj.table, adj.index, agent_id, net.gnn_base, adj.cfg, table_share=share)
    elif isinstance(node_obs, torch.Tensor) and node_obs.dim() == 3 and node_obs.shape[1] > GNN_MAX_NODES:
        nbd = gnn_base_wide(node_obs, adj, agent_id, net.gnn_base)
    else:
        nbd = gnn_base(node_obs, adj, agent_id, net.gnn_base)
    features = mlp_base(nbd if own_obs is None else (own_obs, nbd), net.base)
    if _recurrent(net):
        features, rnn_states = rnn_layer(features, rnn_states, masks, net.rnn)
    return features, rnn_states


def actor_forward(actor, obs, node_obs, adj, agent_id, rnn_states, masks, available_actions=None, deterministic=False, *, dones_prev=None, seed,
                  env_id_base=0, num_agents, draw, draw_dev=None, draw_inc=1, out=None):
    """GR_Actor.forward (graph_actor_critic.py:162-173) -> (actions, action_log_probs, rnn_states), under torch.no_grad().
    obs [rows, obs_dim], node_obs [rows, E, F], adj [rows, E, E] or [rows / S, E, E], agent_id [rows] or [rows, 1], rnn_states [rows, 1, 64],
    masks [rows, 1]: float32 device tensors as the layers take them. available_actions / dones_prev, seed, env_id_base, num_agents, draw, draw_dev,
    draw_inc, out: as for act_head (out may hold "logits"). actions is the int64 [rows, 1] tensor the reference returns; with `out` given and no "actions" in
    it, it is the int32 action_idx [rows] instead (what GmpeEngine.step takes). rnn_states comes back unchanged when the actor has no RNN."""
    with torch.no_grad():
        features, rnn_states = _features(actor, obs, node_obs, adj, agent_id, rnn_states, masks)
        idx, actions, logp = act_head(features, actor.act, available_actions, dones_prev=dones_prev, seed=seed, env_id_base=env_id_base,
                                      num_agents=num_agents, draw=draw, draw_dev=draw_dev, draw_inc=draw_inc, deterministic=deterministic, out=out)
    return (idx if actions is None else actions), logp, rnn_states


def _cent(critic, cent_obs):
    return cent_obs if bool(getattr(getattr(critic, "args", None), "use_cent_obs", True)) else None


def critic_forward(critic, cent_obs, node_obs, adj, agent_id, rnn_states_critic, masks):
    """GR_Critic.forward (graph_actor_critic.py:385-397) -> (values [rows, 1], rnn_states_critic); differentiable where gradients are enabled.
    critic.args.use_cent_obs (default True) decides whether cent_obs enters the MLPBase. v_out is F.linear on the caller's weight and bias — for a
    PopArt v_out that is PopArt.forward. critic_graph_aggr == "node" hands the GNNBase several ids per row, which gnn_base refuses by name."""
    features, rnn_states_critic = _features(critic, _cent(critic, cent_obs), node_obs, adj, agent_id, rnn_states_critic, masks)
    return F.linear(features, critic.v_out.weight, critic.v_out.bias), rnn_states_critic


def _value_head_kind(fn, value_head):
    if value_head not in ("torch", "device"):
        raise ValueError("value_head = %r: %s takes \"torch\" (F.linear) or \"device\" (gmpe.value_head)" % (value_head, fn))
    return value_head == "device"


def minibatch_losses(actor, critic, sample, args, value_normalizer=None, install="replace", workspace=None, shards=None, *, value_head="torch"):
    """evaluate_actions and the loss arithmetic of GR_MAPPO.ppo_update (graph_mappo.py:147-245) for the generators' 16-tuple `sample`: the actor chain up to
    action_logits, the critic chain up to its values — up to its features with args.use_popart —, then ppo_losses (value_normalizer, shards) or
    ppo_losses_popart (critic.v_out, install). Returns their result object unchanged; backward() of its two losses reaches every parameter of the actor
    and of the critic. workspace: the loss call's (ppo_loss.workspace_bytes / popart_workspace_bytes). value_head: "torch" — v_out as F.linear — or
    "device" — a plain nn.Linear v_out through gmpe.value_head, forward and backward; with args.use_popart it changes nothing (ppo_losses_popart
    evaluates v_out itself)."""
    device_value = _value_head_kind("minibatch_losses", value_head)
    if not isinstance(sample, (tuple, list)) or len(sample) != 16:
        raise ValueError("sample must be the generators' 16-tuple")
    share_obs, obs, node_obs, adj, agent_id, share_agent_id, rnn_states, rnn_states_critic = sample[:8]
    masks = sample[11]
    actor_features, _ = _features(actor, obs, node_obs, adj, agent_id, rnn_states, masks)
    logits = action_logits(actor_features, actor.act)
    critic_features, _ = _features(critic, _cent(critic, share_obs), node_obs, adj, share_agent_id, rnn_states_critic, masks)
    if getattr(args, "use_popart", False):
        return ppo_losses_popart(logits, critic_features, sample, args, critic.v_out, install=install, workspace=workspace, shards=shards)
    if device_value:
        values = _value.value_head(critic_features, critic.v_out)
    else:
        values = F.linear(critic_features, critic.v_out.weight, critic.v_out.bias)
    return ppo_losses(logits, values, sample, args, value_normalizer, workspace=workspace, shards=shards)


PPOUpdate = collections.namedtuple("PPOUpdate", ["value_loss", "critic_grad_norm", "policy_loss", "dist_entropy", "actor_grad_norm", "ratio_mean",
                                                  "imp_weights"])
TRAIN_INFO = ("value_loss", "policy_loss", "dist_entropy", "actor_grad_norm", "critic_grad_norm", "ratio")      # graph_mappo.py:309-314


def _graph_kind(fn, graph):
    """train's `graph` -> the generators' adj"""
    if graph not in ("rows", "table"):
        raise ValueError("graph = %r: %s takes \"rows\" (node rows and matrices per minibatch) or \"table\" (the buffer's entity table)" % (graph, fn))
    return "table" if graph == "table" else "matrix"


def _refusals(fn, accumulation_steps, shards):
    """what ppo_update and train refuse, before anything else is read"""
    if shards is not None and not (callable(getattr(shards, "exchange", None)) and hasattr(shards, "world") and hasattr(shards, "rank")):
        raise NotImplementedError("shards: %s takes the exchange of a data-parallel learner — an object with exchange(local), world and rank "
                                  "(gmpe.learner_shards.ProcessGroupExchange); anything else is not supported" % fn)
    if accumulation_steps != 1:
        raise NotImplementedError("accumulation_steps = %r: %s steps at every minibatch (gradient accumulation is not supported)" % (accumulation_steps, fn))


def _ppo_update(actor, critic, actor_optimizer, critic_optimizer, sample, args, value_normalizer, update_actor, install, workspace, shards,
                value_head="torch"):
    """ppo_update -> (PPOUpdate, ratio); ratio: with shards the whole minibatch's imp_weights.mean(), else None (it is u.imp_weights.mean())"""
    res = minibatch_losses(actor, critic, sample, args, value_normalizer, install=install, workspace=workspace, shards=shards, value_head=value_head)
    max_norm = getattr(args, "max_grad_norm", 10.0) if getattr(args, "use_max_grad_norm", True) else None
    actor_optimizer.zero_grad()
    if update_actor:
        res.actor_loss.backward()
    actor_grad_norm = clip_and_step(actor_optimizer, max_norm, parameters=actor.parameters(), step=bool(update_actor), shards=shards)
    critic_optimizer.zero_grad()
    (res.value_loss * getattr(args, "value_loss_coef", 1)).backward()
    scalars = (res.value_loss.detach(), res.policy_loss.detach(), res.dist_entropy.detach(), res.ratio_mean.detach())
    imp_weights = res.imp_weights.detach()
    if shards is None:
        critic_grad_norm, ratio = clip_and_step(critic_optimizer, max_norm, parameters=critic.parameters()), None
    else:                                               # the ranks' contributions, and the sum and the count of imp_weights, ride on the critic's exchange
        extra = torch.stack(scalars + (imp_weights.sum(), imp_weights.new_full((), float(imp_weights.numel()))))
        critic_grad_norm, total = clip_and_step(critic_optimizer, max_norm, parameters=critic.parameters(), shards=shards, extra=extra)
        scalars, ratio = tuple(total[:4].unbind()), total[4] / total[5]
    value_loss, policy_loss, dist_entropy, ratio_mean = scalars
    return PPOUpdate(value_loss, critic_grad_norm, policy_loss, dist_entropy, actor_grad_norm, ratio_mean, imp_weights), ratio


def ppo_update(actor, critic, actor_optimizer, critic_optimizer, sample, args, value_normalizer=None, update_actor=True, install="replace", workspace=None,
               *, accumulation_steps=1, shards=None, value_head="torch"):
    """GR_MAPPO.ppo_update (graph_mappo.py:147-278) in the reference's order: minibatch_losses; actor_optimizer.zero_grad(); with update_actor the actor
    loss's backward(); clip_and_step over actor.parameters() (step only with update_actor); critic_optimizer.zero_grad(); (value_loss *
    args.value_loss_coef).backward(); clip_and_step over critic.parameters(). With args.use_max_grad_norm (default True) the gradients are clipped to
    args.max_grad_norm (default 10.0), else their norm is only reported (the reference's get_grad_norm); args.value_loss_coef defaults to 1.
    The norm and the clip run over net.parameters(), the step over the optimiser's own list, as in the reference: after a PopArt update with
    install="replace" the critic holds new v_out Parameters, which have no gradient, and the optimiser the old ones, which are stepped unclipped.
    Returns PPOUpdate(value_loss, critic_grad_norm, policy_loss, dist_entropy, actor_grad_norm, ratio_mean, imp_weights): detached device scalars and
    the [rows, 1] importance weights; actor_grad_norm is 0 without update_actor. workspace: minibatch_losses' own.
    shards: None, or the exchange of a data-parallel learner (gmpe.learner_shards; no DistributedDataParallel around the networks): `sample` is this
    rank's rows of a minibatch whose other rows lie on the other ranks, with equal parameters everywhere. minibatch_losses(..., shards=shards) gives
    the rank's contributions (reduce="sum"), the two clip_and_step(..., shards=shards) sum the ranks' gradients in rank order and step every replica
    alike, and the rank's value_loss, policy_loss, dist_entropy and ratio_mean ride as `extra` on the critic's exchange (which always happens), so the
    PPOUpdate holds the WHOLE minibatch's scalars and norms, the same bits on every rank; imp_weights stays the rank's own rows. All ranks must make
    the same calls with the same update_actor. args.use_popart with shards is refused by ppo_losses_popart, in its words.
    The reference's GradScaler is not reproduced: with float32 losses it changes no value unless a gradient overflows, and its step() waits for the
    device. accumulation_steps != 1 and a `shards` that is no such exchange raise NotImplementedError, before anything else is read. Nothing here
    waits for the device (the exchange is the caller's). value_head: minibatch_losses'."""
    _refusals("ppo_update", accumulation_steps, shards)
    _value_head_kind("ppo_update", value_head)
    return _ppo_update(actor, critic, actor_optimizer, critic_optimizer, sample, args, value_normalizer, update_actor, install, workspace, shards,
                       value_head)[0]


def train(actor, critic, actor_optimizer, critic_optimizer, buffer, args, value_normalizer=None, update_actor=True, perms=None, *, install="replace",
          accumulation_steps=1, shards=None, value_head="torch", graph="rows"):
    """GR_MAPPO.train (graph_mappo.py:294-359) over a DeviceRolloutBuffer: buffer.normalized_advantages(value_normalizer), then args.ppo_epoch (15) passes
    of the generator the reference chooses — recurrent_generator with args.data_chunk_length (10) under args.use_recurrent_policy (True), else
    naive_recurrent_generator under args.use_naive_recurrent_policy, else feed_forward_generator, each with args.num_mini_batch (1) — and ppo_update
    per sample. perms: None, or one permutation per epoch, handed to the generator's perm= (None: the reference's CPU randperm, uploaded from pinned
    memory; "device": drawn on the device; an int64 tensor is range-checked by the generator, which reads it back: the one wait on this path).
    Returns the reference's train_info: the six sums as float32 device adds in its order (value_loss, policy_loss, dist_entropy, actor_grad_norm,
    critic_grad_norm, ratio = imp_weights.mean()), each divided by ppo_epoch * num_mini_batch — a dict of 0-dim device tensors where the reference
    calls .item() three times per minibatch. Between call and return nothing is copied to the host (a tensor in perms excepted, see above).
    shards: None, or the exchange of a data-parallel learner: `buffer` is this rank's own, the advantages are normalised with the statistics of all
    ranks' buffers (normalized_advantages(value_normalizer, shards=shards)), every minibatch is ppo_update(..., shards=shards), and ratio is the sum
    of all ranks' imp_weights over their count. Every rank must produce the same number of minibatches (the same ppo_epoch and num_mini_batch over
    buffers that yield as many samples): a rank that stops early leaves the others waiting in the exchange. Each rank draws its own permutation.
    value_head: minibatch_losses'.
    graph: "rows" — every minibatch gathers its [rows, E, F] node rows and [rows, E, E] matrices — or "table": the generators run with adj="table" and
    the GNNBase of actor and critic reads the buffer's entity table through one int64 per row (gnn_base_from_table), for a buffer that keeps tables
    (node_form "table" or "both"). The same bits, parameters and train_info, and no faster; what it saves is the minibatch's bytes."""
    _refusals("train", accumulation_steps, shards)
    _value_head_kind("train", value_head)
    adj = _graph_kind("train", graph)
    ppo_epoch, num_mini_batch = int(getattr(args, "ppo_epoch", 15)), int(getattr(args, "num_mini_batch", 1))
    if perms is not None and len(perms) != ppo_epoch:
        raise ValueError("perms must hold one permutation per epoch: %d, not %d" % (ppo_epoch, len(perms)))
    advantages = buffer.normalized_advantages(value_normalizer) if shards is None else buffer.normalized_advantages(value_normalizer, shards=shards)
    info = None
    form = {} if adj == "matrix" else {"adj": adj}          # "rows": the generators are called as before, so any buffer with their signature still serves
    for epoch in range(ppo_epoch):
        perm = None if perms is None else perms[epoch]
        if getattr(args, "use_recurrent_policy", True):
            generator = buffer.recurrent_generator(advantages, num_mini_batch, int(getattr(args, "data_chunk_length", 10)), perm=perm, **form)
        elif getattr(args, "use_naive_recurrent_policy", False):
            if form:
                raise NotImplementedError("graph = \"table\": naive_recurrent_generator yields node rows and matrices only (not supported)")
            generator = buffer.naive_recurrent_generator(advantages, num_mini_batch)
        else:
            generator = buffer.feed_forward_generator(advantages, num_mini_batch, perm=perm, **form)
        for sample in generator:
            u, ratio = _ppo_update(actor, critic, actor_optimizer, critic_optimizer, sample, args, value_normalizer, update_actor, install, None, shards,
                                   value_head)
            terms = (u.value_loss, u.policy_loss, u.dist_entropy, u.actor_grad_norm, u.critic_grad_norm, u.imp_weights.mean() if ratio is None else ratio)
            info = terms if info is None else tuple(a + b for a, b in zip(info, terms))
    if info is None:
        raise ValueError("train needs at least one minibatch: ppo_epoch = %d" % ppo_epoch)
    num_updates = ppo_epoch * num_mini_batch
    return {k: v / num_updates for k, v in zip(TRAIN_INFO, info)}


# ---------------------------------------------------------------------------------------------- one update as a captured graph
_NORM_TENSORS = ("running_mean", "running_mean_sq", "debiasing_term", "weight", "bias", "stddev", "mean", "mean_sq")      # ValueNorm's and PopArt's


def _no_table_rows(fn, sample):
    if any(isinstance(t, TableRows) for t in sample):
        raise NotImplementedError("%s: the sample holds a TableRows (adj=\"table\"): a captured update takes node rows and matrices only — the table form "
                                  "is not supported under capture" % fn)


def _same_sample(fn, static, sample):
    """`sample` must be the 16-tuple the graph was captured for: the same entries, shapes, dtypes and device"""
    if not isinstance(sample, (tuple, list)) or len(sample) != 16:
        raise ValueError("sample must be the generators' 16-tuple")
    for i, (a, b) in enumerate(zip(static, sample)):
        if (a is None) != (b is None):
            raise ValueError("%s: sample[%d] is %s, and the captured graph was built %s it" % (fn, i, "None" if b is None else "given",
                                                                                             "without" if a is None else "with"))
        if a is not None and (not isinstance(b, torch.Tensor) or b.shape != a.shape or b.dtype != a.dtype or b.device != a.device):
            raise ValueError("%s: sample[%d] must be %s %s on %s as at capture, not %s %s on %s — a captured graph is fixed to its shapes (the minibatch "
                             "rows follow from T, N, A, data_chunk_length and num_mini_batch)"
                             % (fn, i, tuple(a.shape), a.dtype, a.device, tuple(getattr(b, "shape", ())), getattr(b, "dtype", type(b).__name__),
                                getattr(b, "device", "the host")))


def _unique(tensors):
    seen, out = set(), []
    for t in tensors:
        if isinstance(t, torch.Tensor) and id(t) not in seen:
            seen.add(id(t))
            out.append(t)
    return out


class CapturedUpdate(object):
    """ppo_update(..., install="in_place") captured once as a torch.cuda.CUDAGraph and replayed: the same kernels on the same inputs in the same order, so
    the same bits, with one host call per minibatch where ppo_update issues about a hundred. The two clip_and_step calls are
    gmpe.optim.ScheduledStep.step(), whose Adam step count lives on the device.

        cap = gmpe.policy.CapturedUpdate(actor, critic, actor_optimizer, critic_optimizer, sample, args, value_normalizer)
        u = cap.update(sample)        # or: train_info = cap.train(buffer)

      sample: a 16-tuple of the generator the updates will come from; only its shapes, dtypes and device matter, and every later sample must have them.
      args, value_normalizer, update_actor, value_head: ppo_update's, fixed at construction. install: "in_place" only — with args.use_popart,
        "replace" creates new Parameters at every update, whose addresses a captured graph cannot follow, and is refused.
      steps_ahead: rows of the two schedules (gmpe.optim.ScheduledStep); update raises RuntimeError before it would run past them, refill() starts
        them again from the optimisers' current param_groups (a decayed lr) and step counts, and train() refills by itself when it has to.
    Construction runs the update twice on a side stream (the warm-up torch.cuda.graph asks for) and once under capture, then puts every tensor the
    update writes back bit for bit: parameters, Adam moments, the ValueNorm / PopArt tensors and the gradients are as before (missing Adam state is
    created as torch creates it: zeros, step 0). Afterwards the .grad of every parameter the losses reach is a fixed tensor that each update overwrites
    (a parameter that had none gets one, zero-filled; replace one and update raises); a parameter they do not reach keeps the .grad it had.
    update(sample) -> the static PPOUpdate: device scalars and imp_weights that the NEXT update overwrites. It copies `sample` into the captured
    tensors, replays and moves the host-side step counts; nothing waits for the device. Everything runs on the current stream, as one linear graph."""

    def __init__(self, actor, critic, actor_optimizer, critic_optimizer, sample, args, value_normalizer=None, update_actor=True, *, install="in_place",
                 value_head="torch", steps_ahead=None):
        if install != "in_place":
            raise NotImplementedError("install = %r: a captured update takes \"in_place\" only — \"replace\" creates new Parameters at every update, "
                                      "whose addresses a captured graph cannot follow (not supported under capture)" % (install,))
        _value_head_kind("CapturedUpdate", value_head)
        _optim._groups(actor_optimizer)
        _optim._groups(critic_optimizer)
        if not isinstance(sample, (tuple, list)) or len(sample) != 16:
            raise ValueError("sample must be the generators' 16-tuple")
        _no_table_rows("CapturedUpdate", sample)
        dev = sample[1].device
        if dev.type != "cuda":
            raise ValueError("the arrays must be CUDA (HIP) device tensors: these kernels have no CPU fallback")
        self.actor, self.critic, self.actor_optimizer, self.critic_optimizer = actor, critic, actor_optimizer, critic_optimizer
        self.args, self.value_normalizer, self.update_actor, self.value_head = args, value_normalizer, bool(update_actor), value_head
        self.max_norm = getattr(args, "max_grad_norm", 10.0) if getattr(args, "use_max_grad_norm", True) else None
        steps_ahead = _optim.STEPS_AHEAD if steps_ahead is None else steps_ahead
        self.sample = tuple(None if t is None else t.detach().clone() for t in sample)
        self._a_all = _unique([p for g in actor_optimizer.param_groups for p in g["params"]] + list(actor.parameters()))
        self._c_all = _unique([p for g in critic_optimizer.param_groups for p in g["params"]] + list(critic.parameters()))
        params = self._a_all + self._c_all
        # everything the update writes, as it is now
        norms = [getattr(o, k, None) for o in (value_normalizer, getattr(critic, "v_out", None)) if o is not None for k in _NORM_TENSORS]
        moments = [st[k] for opt in (actor_optimizer, critic_optimizer) for st in opt.state.values() for k in ("exp_avg", "exp_avg_sq") if k in st]
        old_grads = [p.grad for p in params]
        kept = _unique(params + norms + moments + old_grads)
        with torch.no_grad():
            saved = [t.detach().clone() for t in kept]
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            # the first run finds the tensors the losses reach: their gradients become the fixed ones, the tensor that was .grad before where there was one
            self._backwards(self._losses(), None, None)
            fixed = []
            for p, old in zip(params, old_grads):
                if p.grad is not None and old is not None and old.shape == p.grad.shape and old.dtype == p.grad.dtype and old.device == p.grad.device:
                    p.grad = old
                fixed.append(p.grad)
            self._a_rows = [(p, p.grad) for p in self._a_all if p.grad is not None]
            self._c_rows = [(p, p.grad) for p in self._c_all if p.grad is not None]
            self.actor_step = _optim.ScheduledStep(actor_optimizer, self.max_norm, parameters=actor.parameters(), steps_ahead=steps_ahead) \
                if self.update_actor and self._a_rows else None
            self.critic_step = _optim.ScheduledStep(critic_optimizer, self.max_norm, parameters=critic.parameters(), steps_ahead=steps_ahead)
            self._zero = torch.zeros((), dtype=torch.float32, device=dev)
            self._body()                                # the second run: the captured sequence itself, eagerly
        torch.cuda.current_stream(dev).wait_stream(side)
        created = _unique([st[k] for opt in (actor_optimizer, critic_optimizer) for st in opt.state.values() for k in ("exp_avg", "exp_avg_sq") if k in st])
        have = set(id(t) for t in kept)
        with torch.no_grad():
            for t, v in zip(kept, saved):
                t.copy_(v)
            for t in created + [g for g in fixed if g is not None]:
                if id(t) not in have:
                    t.zero_()
        for s in self._steps():
            s._upload()                                 # row 0 again: the warm-up advanced the counter, not the host's step counts
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.result = self._body()
        for p, old, g in zip(params, old_grads, fixed):
            if g is None:
                p.grad = old                            # not reached by the losses: the .grad it had

    def _steps(self):
        return [s for s in (self.actor_step, self.critic_step) if s is not None]

    def _losses(self):
        return minibatch_losses(self.actor, self.critic, self.sample, self.args, self.value_normalizer, install="in_place", value_head=self.value_head)

    def _backwards(self, res, a_rows, c_rows):
        """ppo_update's two backward passes from gradients that are None, as zero_grad() leaves them; with rows, each new gradient is then copied into
        its fixed tensor, which becomes .grad again, and the step runs -> (actor_grad_norm, critic_grad_norm) (None without rows)"""
        norms = []
        for which, (every, rows, sched) in enumerate(((self._a_all, a_rows, getattr(self, "actor_step", None)),
                                                      (self._c_all, c_rows, getattr(self, "critic_step", None)))):
            for p in every:
                p.grad = None
            if which == 1:
                (res.value_loss * getattr(self.args, "value_loss_coef", 1)).backward()
            elif self.update_actor:
                res.actor_loss.backward()
            if rows is None:
                continue
            if sched is None:                           # the actor without update_actor: clip_grad_norm_ of nothing
                norms.append(self._zero)
                continue
            new = [p.grad for p, _ in rows]
            if any(g is None for g in new):
                raise RuntimeError("a parameter that had a gradient at construction received none in the captured update")
            with torch.no_grad():
                torch._foreach_copy_([g for _, g in rows], new)
            for p, g in rows:
                p.grad = g
            norms.append(sched.step())
        return norms

    def _body(self):
        res = self._losses()
        actor_grad_norm, critic_grad_norm = self._backwards(res, self._a_rows, self._c_rows)
        return PPOUpdate(res.value_loss.detach(), critic_grad_norm, res.policy_loss.detach(), res.dist_entropy.detach(), actor_grad_norm,
                         res.ratio_mean.detach(), res.imp_weights.detach())

    @property
    def remaining(self):
        return min(s.remaining for s in self._steps())

    def update(self, sample):
        _no_table_rows("CapturedUpdate.update", sample)
        _same_sample("CapturedUpdate.update", self.sample, sample)
        for s in self._steps():
            s._budget.need("CapturedUpdate.update")
            s.check_grads()
        with torch.no_grad():
            for dst, src in zip(self.sample, sample):
                if dst is not None:
                    dst.copy_(src)
        self.graph.replay()
        for s in self._steps():
            s.advance_host(1)
        return self.result

    def refill(self):
        for s in self._steps():
            s.refill()

    def train(self, buffer, perms=None):
        """train(..., install="in_place") with every minibatch through update(): its loop, its generators and its train_info, bit for bit.
        normalized_advantages and the generator run eagerly. The schedules are refilled first when param_groups changed since they were filled or when
        fewer than ppo_epoch * num_mini_batch rows are left."""
        args = self.args
        ppo_epoch, num_mini_batch = int(getattr(args, "ppo_epoch", 15)), int(getattr(args, "num_mini_batch", 1))
        if perms is not None and len(perms) != ppo_epoch:
            raise ValueError("perms must hold one permutation per epoch: %d, not %d" % (ppo_epoch, len(perms)))
        if self.remaining < ppo_epoch * num_mini_batch or any(s.stale() for s in self._steps()):
            self.refill()
        advantages = buffer.normalized_advantages(self.value_normalizer)
        info = None
        for epoch in range(ppo_epoch):
            perm = None if perms is None else perms[epoch]
            if getattr(args, "use_recurrent_policy", True):
                generator = buffer.recurrent_generator(advantages, num_mini_batch, int(getattr(args, "data_chunk_length", 10)), perm=perm)
            elif getattr(args, "use_naive_recurrent_policy", False):
                generator = buffer.naive_recurrent_generator(advantages, num_mini_batch)
            else:
                generator = buffer.feed_forward_generator(advantages, num_mini_batch, perm=perm)
            for sample in generator:
                u = self.update(sample)
                terms = (u.value_loss, u.policy_loss, u.dist_entropy, u.actor_grad_norm, u.critic_grad_norm, u.imp_weights.mean())
                info = tuple(t.clone() for t in terms) if info is None else tuple(a + b for a, b in zip(info, terms))      # the next replay overwrites u
        if info is None:
            raise ValueError("train needs at least one minibatch: ppo_epoch = %d" % ppo_epoch)
        num_updates = ppo_epoch * num_mini_batch
        return {k: v / num_updates for k, v in zip(TRAIN_INFO, info)}


# ---------------------------------------------------------------------------------------------- the rollout half
def get_values(critic, share_obs, node_obs, adj, share_agent_id, rnn_states_critic, masks, out=None):
    """GR_MAPPOPolicy.get_values (graphMAPPOPolicy.py) -> values [rows, 1], under torch.no_grad(): the critic chain of critic_forward with value_head
    as v_out. out: value_head's — a float32 device tensor of `rows` elements written in place, e.g. a buffer's value_preds[t]."""
    with torch.no_grad():
        features, _ = _features(critic, _cent(critic, share_obs), node_obs, adj, share_agent_id, rnn_states_critic, masks)
        return _value.value_head(features, critic.v_out, out=out)


def _split_out(fn, out):
    """get_actions' `out` -> (act_head's `out`, the tensor for the values or None)"""
    if out is None:
        return None, None
    if not isinstance(out, dict):
        raise ValueError("out must be a dict: %s takes act_head's entries and \"values\"" % fn)
    out = dict(out)
    return out, out.pop("values", None)


def get_actions(actor, critic, share_obs, obs, node_obs, adj, agent_id, share_agent_id, rnn_states, rnn_states_critic, masks, available_actions=None,
                deterministic=False, *, dones_prev=None, seed, env_id_base=0, num_agents, draw, draw_dev=None, draw_inc=1, out=None):
    """GR_MAPPOPolicy.get_actions (graphMAPPOPolicy.py) -> (values, actions, action_log_probs, rnn_states, rnn_states_critic), the reference's order,
    under torch.no_grad() on the current stream: actor_forward (its chain ends in act_head), then the critic chain ending in value_head.
    The arrays and available_actions / dones_prev, seed, env_id_base, num_agents, draw, draw_dev, draw_inc: as for actor_forward and critic_forward.
    out: actor_forward's dict, which may also hold "values" (value_head's out: float32, `rows` elements, written in place). The states come back
    unchanged from a network without an RNN."""
    act_out, values_out = _split_out("get_actions", out)
    actions, logp, rnn_states = actor_forward(actor, obs, node_obs, adj, agent_id, rnn_states, masks, available_actions, deterministic,
                                              dones_prev=dones_prev, seed=seed, env_id_base=env_id_base, num_agents=num_agents, draw=draw,
                                              draw_dev=draw_dev, draw_inc=draw_inc, out=act_out)
    with torch.no_grad():
        features, rnn_states_critic = _features(critic, _cent(critic, share_obs), node_obs, adj, share_agent_id, rnn_states_critic, masks)
        values = _value.value_head(features, critic.v_out, out=values_out)
    return values, actions, logp, rnn_states, rnn_states_critic


def _rollout_buffer(fn, actor, critic, buffer, returns=False):
    """what the rollout entries need of a DeviceRolloutBuffer, checked before the device is touched"""
    for name in ("engine", "step", "T", "value_preds", "act_outputs", "act_finish"):
        if not hasattr(buffer, name):
            raise ValueError("buffer must be a DeviceRolloutBuffer: %s reads buffer.%s" % (fn, name))
    if buffer.value_preds is None or (returns and buffer.returns is None):
        raise ValueError("%s needs a buffer with value_preds%s (policy_fields)" % (fn, " and returns" if returns else ""))
    table = getattr(buffer, "entity_table", None) is not None          # then a slot's graphs can come from its table (_slot_rows)
    if getattr(buffer, "_node_obs", None) is None and not table:
        raise ValueError("%s reads node_obs rows: the buffer's engine must keep them (node_form 'rows' or 'both')" % fn)
    if getattr(buffer, "_adj", None) is None and not table:
        raise ValueError("%s reads an adjacency: the buffer's engine must keep one (adj_form not 'none')" % fn)
    for net, field in ((actor, "rnn_states"), (critic, "rnn_states_critic")):
        if net is not None and _recurrent(net) and getattr(buffer, field, None) is None:
            raise ValueError("the %s has an RNN: %s needs a buffer with %s (learner_fields)" % ("actor" if field == "rnn_states" else "critic", fn, field))


def _slot_rows(buffer, t):
    """slot t of the buffer's arrays as the networks take them: [N, A, ...] flattened to rows. A buffer that lacks the node rows or the adjacency gives
    the slot's graphs as its [N, W] entity table instead (a TableRows without an index: table row r // A serves row r)"""
    e = buffer.engine
    rows, E = e.N * e.A, int(e.cfg.num_entities)
    flat = lambda x: None if x is None else x[t].reshape((rows,) + tuple(x.shape[3:]))
    if buffer._node_obs is None or buffer._adj is None:
        node_obs, adj = None, TableRows(buffer.entity_table[t], None, e.cfg)
    else:
        node_obs, adj = flat(buffer._node_obs), buffer._adj[t].reshape(-1, E, E)
    return dict(share_obs=flat(buffer.share_obs), obs=flat(buffer.obs), node_obs=node_obs, adj=adj,
                agent_id=flat(buffer.agent_id), share_agent_id=flat(buffer.share_agent_id), rnn_states=flat(buffer.rnn_states),
                rnn_states_critic=flat(buffer.rnn_states_critic), masks=flat(buffer.masks))


def collect_step(actor, critic, buffer, deterministic=False, *, draw_dev=None):
    """One step of run()'s loop (graph_mpe_runner.py:57-103: collect or collect_with_mask, envs.step, insert) on a DeviceRolloutBuffer built with
    policy_fields and learner_fields: get_actions on slot buffer.step — the availability taken from dones[step - 1], everything available at step 0,
    the draw keyed by buffer.act_draw, the values written into value_preds[step], the action and its log-prob into their slots —, then the env step,
    the masks, the step's stop rows and the RNN states of slot step + 1 with the done rows zeroed in one launch (gmpe_step_tail), as
    DeviceRolloutBuffer.act_step does them: ten launches a step. Bit for bit what
    act_step(action_logits(...), value_head(...), rnn_states=..., rnn_states_critic=...) stores from the same layer calls. Nothing is copied to the
    host and nothing waits for the device. Returns the engine's outputs of the step.
    draw_dev: None, or act_head's int64 [1] device counter (buffer.act_draw_counter()): the draw is then keyed by what the counter holds when the
    launch runs, not by the host's buffer.act_draw, and the step's tail launch adds one to it (the sampling launch is given draw_inc = 0, which
    spares its counter launch) — the form a captured step takes (CapturedRollout)."""
    _rollout_buffer("collect_step", actor, critic, buffer)
    t, e = buffer.step, buffer.engine
    c, rows = e.cfg, e.N * e.A
    s = _slot_rows(buffer, t)
    out = buffer.act_outputs()
    out["values"] = buffer.value_preds[t]
    _, _, _, h, hc = get_actions(actor, critic, s["share_obs"], s["obs"], s["node_obs"], s["adj"], s["agent_id"], s["share_agent_id"], s["rnn_states"],
                                 s["rnn_states_critic"], s["masks"], None, deterministic, dones_prev=buffer.dones[t - 1].view(rows) if t else None,
                                 seed=c.seed, env_id_base=c.env_id_base, num_agents=e.A, draw=buffer.act_draw if draw_dev is None else 0,
                                 draw_dev=draw_dev, draw_inc=0 if draw_dev is not None else 1, out=out)
    learner = buffer._learner_inputs(None, None, None, h if _recurrent(actor) else None, hc if _recurrent(critic) else None, "collect_step")
    buffer._tail_draw_dev = draw_dev                        # act_finish's tail launch advances it
    return buffer.act_finish(learner)


def compute(critic, buffer, value_normalizer=None):
    """GMPERunner.compute (graph_mpe_runner.py:431-443): get_values on the last slot, then buffer.compute_returns(next_values, value_normalizer)
    (with args.use_popart the normaliser is critic.v_out, as in the reference's trainer). Returns buffer.returns."""
    _rollout_buffer("compute", None, critic, buffer, returns=True)
    _, use_norm = buffer._flags("compute")
    if use_norm and value_normalizer is None:
        raise ValueError("compute: args.use_valuenorm / use_popart is set, so a value_normalizer is required")
    e = buffer.engine
    s = _slot_rows(buffer, buffer.T)
    next_values = get_values(critic, s["share_obs"], s["node_obs"], s["adj"], s["share_agent_id"], s["rnn_states_critic"], s["masks"])
    return buffer.compute_returns(next_values.view(e.N, e.A, 1), value_normalizer)


def rollout(actor, critic, buffer, value_normalizer=None, deterministic=False):
    """One episode of run()'s loop from buffer.step == 0 (after warmup() or after_update()): buffer.T calls of collect_step, then compute.
    Returns buffer.returns."""
    _rollout_buffer("rollout", actor, critic, buffer, returns=True)
    if buffer.step != 0:
        raise ValueError("rollout starts at buffer.step == 0, not %d (warmup() or after_update() first)" % buffer.step)
    for _ in range(buffer.T):
        collect_step(actor, critic, buffer, deterministic)
    return compute(critic, buffer, value_normalizer)


# ---------------------------------------------------------------------------------------------- one rollout as a captured graph
def _buffer_arrays(buffer):
    """every device tensor the buffer holds, named for a complaint: what a rollout writes lies among them, and a captured one has their addresses
    in its nodes (the buffer enumerates its own: DeviceRolloutBuffer._arrays)"""
    return [("buffer." + k, t) for k, t in buffer._arrays()]


def _capturable_engine(fn, engine, path=True):
    """what a captured rollout refuses of the buffer's engine, by name, from what the host knows; path: the handle's launch path too (fixed at creation)"""
    if getattr(engine, "_timing", False):
        raise NotImplementedError("%s: the engine's timing is enabled (GmpeEngine.timing(True)): its per-launch event pairs have no place in a captured "
                                  "graph — timing(False) first (not supported under capture)" % fn)
    if path and getattr(engine, "adj_form", None) == "full" and engine.tuning()["split"]:
        raise NotImplementedError("%s: this handle runs the split big-E path with a dense adjacency, whose steps fork onto side streams; a captured "
                                  "rollout is one chain on one stream — adj_compact=True or adj_form=\"none\" (not supported under capture)" % fn)


class CapturedRollout(object):
    """rollout(actor, critic, buffer, value_normalizer, deterministic) captured once as a torch.cuda.CUDAGraph and replayed: buffer.T collect_steps and
    compute, unrolled — every step's slot addresses in its own nodes —, the same kernels on the same inputs in the same order, so the same bits, with
    one host call per episode where rollout issues ten launches per step through Python.

        cap = gmpe.policy.CapturedRollout(actor, critic, buffer, value_normalizer)
        returns = cap.replay()        # == rollout(actor, critic, buffer, value_normalizer), bit for bit

      buffer: rollout's, at buffer.step == 0 (after warmup() or after_update()); rows form or table-only. deterministic: collect_step's, fixed here.
    The action draws come from the buffer's device counter (buffer.act_draw_counter()): every captured step keys its draw by the counter and adds one
    to it; replay() first makes the counter equal buffer.act_draw — eager steps may have run since —, launches, adds T to buffer.act_draw, leaves
    buffer.step at 0 and points the engine's current outputs at slot T, as rollout does. Nothing waits for the device.
    Construction runs the rollout once on a side stream (the warm-up torch.cuda.graph asks for; it also gets every kernel's one-time attribute call
    out of the way) and once under capture, which executes nothing, then puts back bit for bit what the warm-up wrote: the engine's state
    (get_state / set_state, which wait for the device), every buffer array, act_draw, step and the engine's bound outputs.
    The graph holds addresses: of every actor and critic parameter, of the value normaliser's tensors and of every buffer array. Values changed in
    place are followed — an optimiser step (torch's Adam, clip_and_step), a ValueNorm update, PopArt with install="in_place" —; a tensor that moved
    is not: replay() compares every data_ptr with the captured one and raises RuntimeError, naming the first that differs, before anything is
    launched. The engine's RNG tape and control override are kernel parameters too: one installed or removed after capture is refused by name.
    Everything runs on the current stream, as one linear graph."""

    def __init__(self, actor, critic, buffer, value_normalizer=None, deterministic=False):
        fn = "CapturedRollout"
        _rollout_buffer(fn, actor, critic, buffer, returns=True)
        _, use_norm = buffer._flags(fn)
        if use_norm and value_normalizer is None:
            raise ValueError("%s: args.use_valuenorm / use_popart is set, so a value_normalizer is required" % fn)
        if buffer.step != 0:
            raise ValueError("%s starts at buffer.step == 0, not %d (warmup() or after_update() first)" % (fn, buffer.step))
        e = buffer.engine
        _capturable_engine(fn, e)
        dev = e.device
        if dev.type != "cuda":
            raise ValueError("the arrays must be CUDA (HIP) device tensors: these kernels have no CPU fallback")
        self.actor, self.critic, self.buffer, self.engine = actor, critic, buffer, e
        self.value_normalizer, self.deterministic = value_normalizer, bool(deterministic)
        self._ovr, self._tape = e._ovr, e._tape
        self.counter = buffer.act_draw_counter()
        buffer.act_outputs()                                # the buffer's own action scratch exists before its arrays are listed
        # everything a rollout writes, as it is now
        state, out, act_draw = e.get_state(), e.out, buffer.act_draw
        kept = _unique([t for _, t in _buffer_arrays(buffer)])
        with torch.no_grad():
            saved = [t.clone() for t in kept]

        def put_back(device):
            """the host's counters and the binding; device: what the warm-up wrote too (a capture moves only the host's side)"""
            if device:
                torch.cuda.current_stream(dev).wait_stream(side)
                e.set_state(state)
                with torch.no_grad():
                    for t, v in zip(kept, saved):
                        t.copy_(v)
            buffer.act_draw, buffer.step = act_draw, 0
            e.rebind(out)

        buffer.sync_act_draw_counter()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        try:
            with torch.cuda.stream(side):
                self._body()                                # the captured sequence itself, eagerly
        finally:
            put_back(True)                                  # also when a layer refused half-way: construction changes nothing the caller can see
        self.graph = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(self.graph):
                self.returns = self._body()
        finally:
            put_back(False)
        self._addresses = [(name, t.data_ptr()) for name, t in self._tensors()]

    def _body(self):
        b = self.buffer
        for _ in range(b.T):
            collect_step(self.actor, self.critic, b, self.deterministic, draw_dev=self.counter)
        return compute(self.critic, b, self.value_normalizer)

    def _tensors(self):
        """(name, tensor) of everything whose address the graph holds, as the modules and the buffer hold them NOW, in a fixed order"""
        out = [("actor." + k, p) for k, p in self.actor.named_parameters()] + [("critic." + k, p) for k, p in self.critic.named_parameters()]
        for tag, o in (("value_normalizer.", self.value_normalizer), ("critic.v_out.", getattr(self.critic, "v_out", None))):
            if o is not None:
                out += [(tag + k, getattr(o, k)) for k in _NORM_TENSORS if isinstance(getattr(o, k, None), torch.Tensor)]
        return out + _buffer_arrays(self.buffer)

    def replay(self):
        fn = "CapturedRollout.replay"
        b, e = self.buffer, self.engine
        if b.step != 0:
            raise ValueError("%s starts at buffer.step == 0, not %d (warmup() or after_update() first)" % (fn, b.step))
        _capturable_engine(fn, e, path=False)
        if e._ovr is not self._ovr:
            raise NotImplementedError("%s: the engine's control override was set or removed after capture: it is a kernel parameter of every captured "
                                      "step — build a new CapturedRollout (not supported under capture)" % fn)
        if e._tape is not self._tape:
            raise NotImplementedError("%s: the engine's RNG tape was set or removed after capture: it is a kernel parameter of every captured step — "
                                      "build a new CapturedRollout (not supported under capture)" % fn)
        now = self._tensors()
        if len(now) != len(self._addresses):
            raise RuntimeError("%s: the graph was captured over %d tensors and the modules and the buffer now hold %d" % (fn, len(self._addresses), len(now)))
        for (name, t), (was, ptr) in zip(now, self._addresses):
            if name != was or t.data_ptr() != ptr:
                raise RuntimeError("%s: %s is not where it was captured (%s): the graph reads and writes the captured address — keep tensors in place "
                                   "(torch's Adam, clip_and_step and PopArt's install=\"in_place\" do), or build a new CapturedRollout"
                                   % (fn, was, "now %s" % name if name != was else "data_ptr 0x%x, captured 0x%x" % (t.data_ptr(), ptr)))
        if not e.h:
            raise RuntimeError("%s: the engine was closed" % fn)
        b.sync_act_draw_counter()
        self.graph.replay()
        b.act_draw += b.T
        b._bind(b.T)
        return self.returns


def _captured_refusals(fn, keywords):
    """what run(..., captured=True) refuses of its iteration keywords, as CapturedUpdate refuses them -> the keywords with install filled in"""
    kw = dict(keywords)
    install = kw.setdefault("install", "in_place")
    if install != "in_place":
        raise NotImplementedError("install = %r: %s with captured=True takes \"in_place\" only — \"replace\" creates new Parameters at every update, "
                                  "whose addresses a captured graph cannot follow (not supported under capture)" % (install, fn))
    if kw.get("shards") is not None:
        raise NotImplementedError("shards: %s with captured=True runs one unsharded learner — the exchange between the ranks is no part of a captured "
                                  "update (not supported under capture)" % fn)
    if kw.get("graph", "rows") != "rows":
        raise NotImplementedError("graph = %r: %s with captured=True takes \"rows\" only — a captured update takes node rows and matrices, the table "
                                  "form is not supported under capture" % (kw["graph"], fn))
    return kw


class _CapturedIteration(object):
    """iteration(...) with both halves replayed: the rollout through a CapturedRollout built at the first call, train through a CapturedUpdate built
    from the first minibatch of the first episode — drawn with the generator's own permutation and the CPU generator put back, so that train draws
    the same one again. Bit for bit iteration(..., install="in_place")."""

    def __init__(self, actor, critic, actor_optimizer, critic_optimizer, buffer, args, value_normalizer, update_actor=True, perms=None, *,
                 deterministic=False, install="in_place", accumulation_steps=1, shards=None, value_head="torch", graph="rows"):
        _refusals("run", accumulation_steps, shards)
        _value_head_kind("run", value_head)
        self.nets = (actor, critic, actor_optimizer, critic_optimizer)
        self.buffer, self.args, self.value_normalizer = buffer, args, value_normalizer
        self.update_actor, self.perms, self.deterministic, self.value_head = update_actor, perms, deterministic, value_head
        self.rollout = self.update = None

    def _first_sample(self):
        buffer, args = self.buffer, self.args
        num_mini_batch = int(getattr(args, "num_mini_batch", 1))
        perm = None if self.perms is None else self.perms[0]
        advantages = buffer.normalized_advantages(self.value_normalizer)
        rng = torch.get_rng_state()
        if getattr(args, "use_recurrent_policy", True):
            generator = buffer.recurrent_generator(advantages, num_mini_batch, int(getattr(args, "data_chunk_length", 10)), perm=perm)
        elif getattr(args, "use_naive_recurrent_policy", False):
            generator = buffer.naive_recurrent_generator(advantages, num_mini_batch)
        else:
            generator = buffer.feed_forward_generator(advantages, num_mini_batch, perm=perm)
        sample = next(iter(generator))
        torch.set_rng_state(rng)
        return sample

    def __call__(self):
        actor, critic = self.nets[:2]
        buffer = self.buffer
        if self.rollout is None:
            self.rollout = CapturedRollout(actor, critic, buffer, self.value_normalizer, self.deterministic)
        self.rollout.replay()
        if self.update is None:
            self.update = CapturedUpdate(*self.nets, self._first_sample(), self.args, self.value_normalizer, self.update_actor, install="in_place",
                                         value_head=self.value_head)
        info = self.update.train(buffer, self.perms)
        info["average_episode_rewards"] = buffer.rewards.mean() * buffer.T
        buffer.after_update()
        return info


def iteration(actor, critic, actor_optimizer, critic_optimizer, buffer, args, value_normalizer=None, update_actor=True, perms=None, *,
              deterministic=False, install="replace", accumulation_steps=1, shards=None, value_head="torch", graph="rows"):
    """One iteration of run() (graph_mpe_runner.py:57-129): rollout, train, buffer.after_update(). Returns train's dict plus
    average_episode_rewards = buffer.rewards.mean() * buffer.T (graph_mpe_runner.py:117), a 0-dim device tensor like the others.
    update_actor, perms, install, accumulation_steps, shards, value_head, graph: train's; deterministic: collect_step's."""
    _refusals("iteration", accumulation_steps, shards)
    _value_head_kind("iteration", value_head)
    _graph_kind("iteration", graph)
    rollout(actor, critic, buffer, value_normalizer, deterministic)
    info = train(actor, critic, actor_optimizer, critic_optimizer, buffer, args, value_normalizer, update_actor, perms, install=install,
                 accumulation_steps=accumulation_steps, shards=shards, value_head=value_head, graph=graph)
    info["average_episode_rewards"] = buffer.rewards.mean() * buffer.T
    buffer.after_update()
    return info


# ---------------------------------------------------------------------------------------------- run(): the periodic eval, and the loop itself
def eval_episode(actor, eval_engine, args=None, *, episode_length=None, seed=0):
    """GMPERunner.eval (graph_mpe_runner.py:445-516): one deterministic episode on the eval envs, under torch.no_grad(). eval_engine: a GmpeEngine (or a
    vec env's .engine) of its own, with node rows and an adjacency. A reset, then episode_length (keyword, else args.episode_length, else the engine's
    cfg.episode_length) times: actor_forward(..., deterministic=True, available_actions=None) on the engine's outputs with this function's own
    [N, A, recurrent_N, hidden_size] states (args' sizes, default 1 and 64) and [N, A, 1] masks, the env step, and one launch of gmpe_eval_step: the
    reward sums, and masks and RNN states reset per ENV — zero where every agent of the env is done — as the reference does; there are no stop-action
    rows and a finished env is not frozen (the engine's auto-reset plays on, as the reference's eval envs do).
    Returns {'eval_average_episode_rewards': float64 [N, A] sums over the steps, 'mean': 0-dim float64, log_env's np.mean of them}: device tensors,
    bit for bit the reference's NumPy on the same rewards. Nothing is copied to the host and nothing waits for the device."""
    eng = eval_engine if hasattr(eval_engine, "out") else getattr(eval_engine, "engine", None)
    if eng is None or not hasattr(eng, "out") or not hasattr(eng, "cfg"):
        raise ValueError("eval_episode: eval_engine must be a GmpeEngine (or a BatchedGraphMPEVecEnv's .engine), not %s" % type(eval_engine).__name__)
    if eng.out.node_obs is None:
        raise ValueError("eval_episode reads node_obs rows: eval_engine must keep them (node_form 'rows' or 'both')")
    if eng.out.adj is None:
        raise ValueError("eval_episode reads an adjacency: eval_engine must keep one (adj_form not 'none')")
    cfg = eng.cfg
    T = episode_length if episode_length is not None else getattr(args, "episode_length", None)
    T = int(cfg.episode_length if T is None else T)
    if T < 1:
        raise ValueError("eval_episode: episode_length must be >= 1, not %d" % T)
    N, A = eng.N, eng.A
    rows, dev = N * A, eng.device
    R, H = int(getattr(args, "recurrent_N", 1)), int(getattr(args, "hidden_size", 64))
    with torch.no_grad():
        o = eng.reset()
        E = int(o.node_obs.shape[-2])
        rnn_states = torch.zeros((N, A, R, H), dtype=torch.float32, device=dev)
        masks = torch.ones((N, A, 1), dtype=torch.float32, device=dev)
        sums = torch.empty((N, A), dtype=torch.float64, device=dev)
        flat_h = rnn_states.view(rows, R, H)
        for t in range(T):
            idx, _, h = actor_forward(actor, o.obs.reshape(rows, -1), o.node_obs.reshape(rows, E, -1), o.adj.reshape(-1, E, E), o.agent_id.reshape(rows),
                                      flat_h, masks.view(rows, 1), None, True, seed=seed, env_id_base=int(cfg.env_id_base), num_agents=A, draw=t, out={})
            if h is not flat_h:
                flat_h.copy_(h.reshape(flat_h.shape))
            o = eng.step(idx.view(N, A))
            _infos.eval_step(o.reward, o.done, sums, masks, rnn_states, first=t == 0)
        mean = _infos.eval_mean(sums)
    return {"eval_average_episode_rewards": sums, "mean": mean}


def linear_lr(initial_lr, episode, episodes):
    """update_linear_schedule's learning rate (onpolicy/utils/util.py:18-22), in its arithmetic"""
    return initial_lr - (initial_lr * (episode / float(episodes)))


def run(actor, critic, actor_optimizer, critic_optimizer, buffer, args, value_normalizer=None, *, episodes=None, eval_engine=None, on_log=None,
        on_eval=None, on_save=None, eval_seed=0, captured=False, **iteration_keywords):
    """GMPERunner.run (graph_mpe_runner.py:40-207) over a DeviceRolloutBuffer: buffer.warmup(), then `episodes` iterations (default
    int(args.num_env_steps) // episode_length // n_rollout_threads; episode_length is args.episode_length, else buffer.T; n_rollout_threads is
    args.n_rollout_threads, else the engine's N). Per episode, in the reference's order:
      with args.use_linear_lr_decay, GR_MAPPOPolicy.lr_decay: every param_group of actor_optimizer gets linear_lr(args.lr, episode, episodes), of
        critic_optimizer linear_lr(args.critic_lr, episode, episodes);
      iteration(actor, critic, actor_optimizer, critic_optimizer, buffer, args, value_normalizer, **iteration_keywords);
      total_num_steps = (episode + 1) * episode_length * n_rollout_threads;
      on_save(episode) when episode % args.save_interval == 0 or on the last episode;
      on_log(total_num_steps, train_infos, env_infos) when episode % args.log_interval == 0: iteration's dict (average_episode_rewards included) and
        gmpe.env_infos(buffer, args) of the rollout's last step;
      on_eval(total_num_steps, eval_infos) when episode % args.eval_interval == 0 and args.use_eval: eval_episode(actor, eval_engine, args, seed=eval_seed).
    After the loop on_save(episodes - 1) once more: the reference's final forced save. The intervals default to the reference's 1, 5 and 25. A callback
    that is None is skipped, and what only it would receive is not computed. Every payload is device tensors: run itself never waits for the device,
    a callback that reads a value does. args.increase_fairness is refused: the engine's reward weights are fixed at creation. args.use_eval without
    eval_engine raises ValueError. Returns the last iteration's train_infos (None with no episode).
    captured=True: both halves of every iteration are replayed graphs — after warmup() a CapturedRollout is built and every episode's rollout is its
    replay(); every train is CapturedUpdate.train, the CapturedUpdate built from the first minibatch of the first episode; the lr decay reaches the
    update through the schedules' refill. Bit for bit run(..., install="in_place"), and install defaults to "in_place" then: any other install, shards
    and graph="table" raise NotImplementedError, before anything else is read. Still nothing waits for the device but the two constructions, in
    the first episode."""
    if captured:
        iteration_keywords = _captured_refusals("run", iteration_keywords)
    if getattr(args, "increase_fairness", False):
        raise NotImplementedError("args.increase_fairness: run() cannot raise fair_rew mid-training — the engine's reward weights are fixed at "
                                  "creation (not supported)")
    use_eval = bool(getattr(args, "use_eval", False))
    if use_eval and eval_engine is None:
        raise ValueError("args.use_eval is set: run needs eval_engine (a GmpeEngine of its own for the eval episodes)")
    episode_length = int(getattr(args, "episode_length", None) or buffer.T)
    threads = int(getattr(args, "n_rollout_threads", None) or buffer.engine.N)
    if episodes is None:
        if getattr(args, "num_env_steps", None) is None:
            raise ValueError("run needs episodes= or args.num_env_steps")
        episodes = int(args.num_env_steps) // episode_length // threads
    episodes = int(episodes)
    save_interval, log_interval = int(getattr(args, "save_interval", 1)), int(getattr(args, "log_interval", 5))
    eval_interval = int(getattr(args, "eval_interval", 25))
    decay = bool(getattr(args, "use_linear_lr_decay", False))
    if decay and (getattr(args, "lr", None) is None or getattr(args, "critic_lr", None) is None):
        raise ValueError("args.use_linear_lr_decay is set: run needs args.lr and args.critic_lr, the rates the schedule starts from")
    replayed = _CapturedIteration(actor, critic, actor_optimizer, critic_optimizer, buffer, args, value_normalizer, **iteration_keywords) \
        if captured else None
    buffer.warmup()
    train_infos = None
    for episode in range(episodes):
        if decay:
            for optimizer, initial in ((actor_optimizer, args.lr), (critic_optimizer, args.critic_lr)):
                for group in optimizer.param_groups:
                    group["lr"] = linear_lr(initial, episode, episodes)
        if replayed is not None:
            train_infos = replayed()
        else:
            train_infos = iteration(actor, critic, actor_optimizer, critic_optimizer, buffer, args, value_normalizer, **iteration_keywords)
        total_num_steps = (episode + 1) * episode_length * threads
        if on_save is not None and (episode % save_interval == 0 or episode == episodes - 1):
            on_save(episode)
        if on_log is not None and episode % log_interval == 0:
            on_log(total_num_steps, train_infos, _infos.env_infos(buffer, args))
        if on_eval is not None and use_eval and episode % eval_interval == 0:
            on_eval(total_num_steps, eval_episode(actor, eval_engine, args, seed=eval_seed))
    if on_save is not None:
        on_save(episodes - 1)
    return train_infos


def evaluator_act(actor, evaluator, deterministic=True, seed=0, draw0=0):
    """The act(obs, node_obs, adj, agent_id, masks, available_actions) -> int32 [N, A] callable BatchedEvaluator documents, from `actor`:
    [N, A, ...] flattened to rows, evaluator.rnn_states (when the evaluator carries them, [N, A, 1, 64]) read and written in place, `draw` advanced by one
    per call from draw0, the adjacency in either form the engine hands out ([N, E, E] or [N, A, E, E]). It always runs under torch.no_grad()."""
    cfg = evaluator.engine.cfg
    N, A = evaluator.N, evaluator.A
    rows = N * A
    state = {"draw": int(draw0)}
    if _recurrent(actor) and evaluator.rnn_states is None:
        raise ValueError("the actor has an RNN: build the evaluator with rnn_states=[N, A, 1, 64] so that record() resets them")

    def act(obs, node_obs, adj, agent_id, masks, available_actions):
        if adj is None:
            raise ValueError("the engine hands out no adjacency (adj_form='none'): evaluator_act needs one")
        E = int(node_obs.shape[-2])
        hxs = evaluator.rnn_states
        flat_h = None if hxs is None else hxs.reshape(rows, hxs.shape[2], hxs.shape[3])
        idx, _, h = actor_forward(actor, obs.reshape(rows, -1), node_obs.reshape(rows, E, -1), adj.reshape(-1, E, E), agent_id.reshape(rows),
                                  flat_h, masks.reshape(rows, 1), available_actions.reshape(rows, -1), deterministic, seed=seed,
                                  env_id_base=int(cfg.env_id_base), num_agents=A, draw=state["draw"], out={})
        state["draw"] += 1
        if hxs is not None and h is not flat_h:
            hxs.copy_(h.reshape(hxs.shape))
        return idx.view(N, A)

    return act
