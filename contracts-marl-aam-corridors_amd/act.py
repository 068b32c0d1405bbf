"""The rollout half of the discrete action head on the device (include/gmpe.h gmpe_act_sample): logits in, one action and its log-prob per row out.

    logits = actor.act.action_out.linear(actor_features)              # the head's linear layer, before Categorical masks it
    action_idx, actions, action_log_probs = gmpe.sample_actions(logits, available_actions, seed=cfg.seed, env_id_base=cfg.env_id_base,
                                                                num_agents=cfg.num_agents, draw=step_counter)

One launch does what ACTLayer.forward does in about eight torch ops (onpolicy/algorithms/utils/act.py:107-113: the masked Categorical of
distributions.py:84-91, sample() or mode(), log_probs) and what the runner then does to the action for the env and the buffer
(graph_mpe_runner.py:299-320, 356-377). Two properties torch's ops do not give:
  * action_log_probs are bit for bit what ppo_losses recomputes for the same logits, availability and action: an unchanged policy has ratio exactly 1;
  * the draw of a row is keyed by (seed, its env's global id, its agent, draw) on the env streams' Philox generator, so the actions do not depend on how
    the envs are spread over calls, handles, devices or ranks.
There is no torch fallback: the arrays must be on a HIP device. DeviceRolloutBuffer.act_step puts this launch in front of the env step.
"""
import ctypes as C

import torch

from . import _lib
from .engine import _need_cuda, _ordinal, _stream_of
from .ppo_loss import _available, _logits_shape, _widened

OUT_KEYS = ("action_idx", "actions", "actions_f32", "action_log_probs")
_OUT_DTYPES = dict(action_idx=torch.int32, actions=torch.int64, actions_f32=torch.float32, action_log_probs=torch.float32)


def _rows_tensor(name, t, rows, dev, dtypes, anchor="logits"):
    if not isinstance(t, torch.Tensor) or t.dtype not in dtypes or t.numel() != rows or not t.is_contiguous():
        raise ValueError("%s must be a contiguous %s tensor with %d elements" % (name, " or ".join(str(d) for d in dtypes), rows))
    if t.device != dev:
        raise ValueError("%s must be on %s (the device of %s)" % (name, dev, anchor))
    return t


def _plan(rows, K, dev, anchor, available_actions, dones_prev, stop_action, seed, env_id_base, num_agents, draw, draw_dev, draw_inc, deterministic, out,
          more_out=()):
    """What sample_actions and head.act_head share: every argument besides the logits (or the features in their place; `anchor` names them in a
    complaint) checked, the outputs taken from `out` or allocated -> (the plan without its logits, (action_idx, actions, action_log_probs), out as a
    dict, the availability the plan points to: keep it until the launch is queued). more_out: {key: (dtype, elements)} of further entries `out` may hold; they are checked and left to the caller."""
    if available_actions is not None and dones_prev is not None:
        raise ValueError("available_actions and dones_prev are two sources of the availability: give at most one")
    if available_actions is not None:
        available_actions = _available(available_actions, rows, K, dev, contiguous=True)
    if dones_prev is not None:
        _rows_tensor("dones_prev", dones_prev, rows, dev, (torch.uint8, torch.bool), anchor)
    elif stop_action is not None:
        raise ValueError("stop_action is read with dones_prev only")
    stop = K // 2 if stop_action is None else int(stop_action)          # available_actions[int(n / 2)] = 1 (graph_mpe_runner.py:283)
    if not 0 <= stop < K:
        raise ValueError("stop_action must lie in [0, %d)" % K)
    num_agents = int(num_agents)
    if num_agents < 1:
        raise ValueError("num_agents must be >= 1")
    if not -2 ** 31 <= int(env_id_base) < 2 ** 31:
        raise ValueError("env_id_base must fit 32 bits")
    if int(draw) < 0 or int(draw_inc) < 0:
        raise ValueError("draw and draw_inc must be >= 0")
    if draw_dev is not None:
        if not isinstance(draw_dev, torch.Tensor) or draw_dev.dtype not in (torch.int64, torch.uint64) or draw_dev.numel() != 1 or \
                not draw_dev.is_contiguous():
            raise ValueError("draw_dev must be a contiguous int64 tensor with one element")
        if draw_dev.device != dev:
            raise ValueError("draw_dev must be on %s (the device of %s)" % (dev, anchor))
    given = dict(out or {})
    keys = OUT_KEYS + tuple(more_out)
    unknown = set(given) - set(keys)
    if unknown:
        raise ValueError("unknown out entries: %s (expected some of %s)" % (sorted(unknown), list(keys)))
    for k, t in given.items():
        dtype, n = more_out[k] if k in more_out else (_OUT_DTYPES[k], rows)
        _rows_tensor("out[%r]" % k, t, n, dev, (dtype,), anchor)
    _need_cuda(dev)
    idx = given.get("action_idx")
    if idx is None:
        idx = torch.empty((rows,), dtype=torch.int32, device=dev)
    logp = given.get("action_log_probs")
    if logp is None:
        logp = torch.empty((rows, 1), dtype=torch.float32, device=dev)
    act64 = given.get("actions")
    if act64 is None and out is None:
        act64 = torch.empty((rows, 1), dtype=torch.int64, device=dev)
    actf = given.get("actions_f32")
    plan = _lib.GmpeActPlan()
    plan.rows, plan.n_actions, plan.num_agents, plan.stop_action, plan.deterministic = rows, K, num_agents, stop, int(bool(deterministic))
    plan.env_id_base, plan.seed = int(env_id_base), int(seed) & 0xFFFFFFFFFFFFFFFF
    plan.draw, plan.draw_inc = int(draw) & 0xFFFFFFFFFFFFFFFF, int(draw_inc) & 0xFFFFFFFFFFFFFFFF
    plan.draw_dev = None if draw_dev is None else draw_dev.data_ptr()
    plan.available_actions = None if available_actions is None else available_actions.data_ptr()
    plan.dones_prev = None if dones_prev is None else dones_prev.data_ptr()
    plan.action_idx, plan.log_probs = idx.data_ptr(), logp.data_ptr()
    plan.actions_f32 = None if actf is None else actf.data_ptr()
    plan.actions_i64 = None if act64 is None else act64.data_ptr()
    return plan, (idx, act64, logp), given, available_actions


def sample_actions(logits, available_actions=None, *, dones_prev=None, stop_action=None, seed, env_id_base=0, num_agents, draw, draw_dev=None,
                   draw_inc=1, deterministic=False, out=None, stream=None):
    """ACTLayer.forward for a single Discrete head, one launch (gmpe_act_sample): returns (action_idx int32 [rows] — what GmpeEngine.step takes —,
    actions int64 [rows, 1], action_log_probs float32 [rows, 1]), rows = N*A in the policy's [env, agent] order.
      logits: float32 [rows, n_actions <= 64], contiguous, on the device (float16 / bfloat16 are widened first).
      availability, from at most one source: available_actions float32 [rows, n_actions] (non-zero = available); or dones_prev uint8 / bool [rows] with
        stop_action (default n_actions // 2) — a row whose dones_prev is set may only take stop_action, the training loop's rule
        (graph_mpe_runner.py:270-286), without a [rows, n_actions] array; or neither: everything is available.
      seed, env_id_base, num_agents: the engine's config (cfg.seed, cfg.env_id_base, cfg.num_agents); row r is agent r % num_agents of env
        env_id_base + r // num_agents. draw: a counter, one value per act. draw_dev: an int64 [1] device tensor; the rows then use draw_dev + draw and
        the call adds draw_inc to it on the stream, so a captured graph draws fresh numbers at every replay.
      deterministic=True: FixedCategorical.mode, the first index of the largest masked logit; an evaluator's `act` callable can use it.
      out: optional dict with some of action_idx (int32), actions (int64), actions_f32 (float32), action_log_probs (float32), each contiguous with
        `rows` elements on the device — e.g. views into a rollout buffer's slots — written in place; action_idx and action_log_probs are allocated
        when absent, and with `out` given the int64 actions are written (and returned, else None) only when it holds "actions".
      stream: a torch.cuda.Stream (default: the current one). Nothing here waits for the device."""
    if isinstance(logits, (tuple, list)) or (isinstance(logits, torch.Tensor) and logits.dim() > 2):
        shape = tuple(logits.shape) if isinstance(logits, torch.Tensor) else "a list of %d heads" % len(logits)
        raise NotImplementedError("logits of shape %s: only a single Discrete head is supported (MultiDiscrete, mixed and continuous heads are not)"
                                  % (shape,))
    dev, rows, K = _logits_shape(logits)
    if not logits.is_contiguous():
        raise ValueError("logits must be contiguous")
    logits = _widened(logits)
    if logits.dtype != torch.float32:
        raise ValueError("logits must be float32 (or float16 / bfloat16, widened here)")
    plan, outs, _, keep = _plan(rows, K, dev, "logits", available_actions, dones_prev, stop_action, seed, env_id_base, num_agents, draw, draw_dev, draw_inc,
                                deterministic, out)
    plan.logits = logits.data_ptr()
    st = C.c_void_p(stream.cuda_stream) if stream is not None else _stream_of(dev)
    _lib.check(_lib.load().gmpe_act_sample(_ordinal(dev), C.byref(plan), st), "gmpe_act_sample")
    del keep                                            # the availability as the launch reads it lives until the launch is queued
    return outs
