"""What run()'s log and eval intervals compute, on device data: Runner.process_infos + log_env (onpolicy/runner/shared/base_runner.py:194-302) and the
bookkeeping of GMPERunner.eval (graph_mpe_runner.py:445-516).

    env_infos(source)   ->  {'agent0/individual_rewards': 0-dim float64 device tensor, 'agent0/time_to_goal': ..., ...}
    eval_step(...)      ->  one launch behind each env step of the eval episode: reward sums, per-env masks, zeroed RNN rows
    eval_mean(sums)     ->  log_env's np.mean of the finished [N, A] sums

Every value is bit for bit what float64 NumPy gives the reference: np.mean of a list sums consecutive chunks of 8192 values, each by pairwise_sum,
in order, from +0.0 (gmpe_infos.hip). Nothing is copied to the host and nothing waits for the device.

`dt` defaults to the world's dt (engine.cfg.dt): the reference's `self.dt` (base_runner.py:216) is never assigned ("the `dt` finding").
"""
import collections
import ctypes as C

import torch

from . import _lib
from .config import INFO_KEYS

# process_infos' names in the order it fills its dict (base_runner.py:252-288) -> the info column each list is built from; formation_dist has no
# column (no scenario writes 'Formation_dist') and process_infos reads no 'Phase_reached', so log_env never logs either.
ENV_INFO_NAMES = (("individual_rewards", "individual_reward"), ("time_to_goal", "Time_req_to_goal"), ("min_time_to_goal", "Min_time_to_goal"),
                  ("dist_to_goal", "Dist_to_goal"), ("num_agent_collisions", "Num_agent_collisions"), ("num_obstacle_collisions", "Num_obst_collisions"),
                  ("distance_mean", "Distance_mean"), ("distance_variance", "Distance_variance"), ("mean_variance", "Mean_by_variance"),
                  ("dists_traveled", "Dists_traveled"), ("time_taken", "Time_taken"), ("time_mean", "Time_mean"), ("time_variance", "Time_stddev"),
                  ("time_mn_by_stddev", "Time_mean_by_stddev"), ("conformance_percentages", "Conformance"), ("delta_space", "Delta_spacing"),
                  ("spacing_violations", "Spacing_violations"))


_KEYS = {}


def env_info_keys(num_agents, include_min_time=True):
    """[('agent{a}/<name>', a, info column)] in process_infos' order, without the keys whose list would be empty"""
    k = (int(num_agents), bool(include_min_time))
    if k not in _KEYS:
        _KEYS[k] = tuple(("agent%d/%s" % (a, name), a, INFO_KEYS.index(key)) for a in range(k[0]) for name, key in ENV_INFO_NAMES
                         if k[1] or key != "Min_time_to_goal")
    return list(_KEYS[k])


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _device_tensor(fn, name, t, dtype, shape=None):
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s: %s must be a torch tensor, not %s" % (fn, name, type(t).__name__))
    if t.device.type != "cuda":
        raise ValueError("%s: %s must be a CUDA (HIP) device tensor: this kernel has no CPU fallback" % (fn, name))
    if t.dtype != dtype or not t.is_contiguous() or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError("%s: %s must be a contiguous %s tensor%s, not %s %s" % (fn, name, dtype, "" if shape is None else " of shape %s" % (tuple(shape),),
                                                                                  t.dtype, tuple(t.shape)))
    return t


def _source(source):
    """(info tensor or None, engine or None, buffer's T or None, what the source is called)"""
    if isinstance(source, torch.Tensor):
        return source, None, None, "source"
    if hasattr(source, "info") and hasattr(source, "engine"):                        # a DeviceRolloutBuffer
        return source.info, source.engine, getattr(source, "T", None), "buffer.info"
    eng = source if hasattr(source, "out") else getattr(source, "engine", None)       # a GmpeEngine, or a vec env's .engine
    if eng is None or not hasattr(eng, "out"):
        raise ValueError("env_infos: source must be a DeviceRolloutBuffer, a GmpeEngine or the [N, A, %d] info tensor, not %s"
                         % (len(INFO_KEYS), type(source).__name__))
    return eng.out.info, eng, None, "engine.out.info"


def env_infos(source, args=None, *, episode_length=None, dt=None, include_min_time=None, out=None):
    """Runner.process_infos(infos) + log_env's np.mean per key (base_runner.py:194-302) from the info rows of the last step, on the device:
    an ordered dict 'agent{a}/<name>' -> 0-dim float64 device tensor, the names and their order process_infos', each tensor a view of one [A, 18] result.
    source: a DeviceRolloutBuffer (its .info: the rows of the rollout's last step), a GmpeEngine (.out.info) or the float32 [N, A, 18] tensor itself.
    A Time_req_to_goal of -1 counts as episode_length * dt: episode_length from the keyword, else args.episode_length, else the buffer's T, else
    the engine's cfg.episode_length; dt from the keyword, else the engine's cfg.dt. Keys whose list would be empty are left out as log_env skips
    them: min_time_to_goal unless cfg.max_speed > 0 (include_min_time overrides; a bare tensor defaults to True), formation_dist and Phase_reached
    always. out: an optional float64 [A, 18] device tensor for the result. One launch (gmpe_env_infos) on the current stream."""
    fn = "env_infos"
    info, eng, buf_T, what = _source(source)
    if info is None:
        raise ValueError("env_infos: %s is None — the engine was built without info (GmpeEngine(..., with_info=True))" % what)
    cfg = getattr(eng, "cfg", None)
    if episode_length is None:
        episode_length = getattr(args, "episode_length", None)
    if episode_length is None:
        episode_length = buf_T if buf_T is not None else getattr(cfg, "episode_length", None)
    if episode_length is None:
        raise ValueError("env_infos: episode_length is required with a bare info tensor (keyword, or args.episode_length)")
    if dt is None:
        dt = getattr(cfg, "dt", None)
    if dt is None:
        raise ValueError("env_infos: dt is required with a bare info tensor (the world's dt)")
    if include_min_time is None:
        include_min_time = True if cfg is None else cfg.max_speed > 0
    if not isinstance(info, torch.Tensor) or info.dim() != 3 or info.shape[2] != len(INFO_KEYS):
        raise ValueError("env_infos: %s must be a float32 [N, A, %d] tensor" % (what, len(INFO_KEYS)))
    N, A = int(info.shape[0]), int(info.shape[1])
    _device_tensor(fn, what, info, torch.float32)
    if out is None:
        out = torch.empty((A, len(INFO_KEYS)), dtype=torch.float64, device=info.device)
    else:
        _device_tensor(fn, "out", out, torch.float64, (A, len(INFO_KEYS)))
    plan = _lib.GmpeEnvInfosPlan(N, A, int(episode_length), 0, float(dt), info.data_ptr(), out.data_ptr())
    _lib.check(_lib.load().gmpe_env_infos(info.device.index, C.byref(plan), _stream(info.device)), "gmpe_env_infos")
    cells = out.view(-1).unbind(0)                           # every 0-dim view in one call: a view per key costs more than the launch
    return collections.OrderedDict((name, cells[a * len(INFO_KEYS) + col]) for name, a, col in env_info_keys(A, include_min_time))


def eval_step(reward, done, sums, masks, rnn_states=None, first=False):
    """One step of GMPERunner.eval's bookkeeping (graph_mpe_runner.py:492-505) in one launch (gmpe_eval_step) on the current stream:
    sums [N, A] float64 += reward [N, A] float32 (first: stored, so `sums` needs no zeroing); masks [N, A, 1] float32 = 0 for every agent of an env
    whose agents are all done (done [N, A] uint8 or bool), else 1; the rows rnn_states[n] of such an env ([N, A, R, H] float32, optional) zeroed."""
    fn = "eval_step"
    _device_tensor(fn, "reward", reward, torch.float32)
    if reward.dim() != 2:
        raise ValueError("eval_step: reward must be [N, A], not %s" % (tuple(reward.shape),))
    N, A = int(reward.shape[0]), int(reward.shape[1])
    if isinstance(done, torch.Tensor) and done.dtype == torch.bool:
        done = done.view(torch.uint8)
    _device_tensor(fn, "done", done, torch.uint8, (N, A))
    _device_tensor(fn, "sums", sums, torch.float64, (N, A))
    _device_tensor(fn, "masks", masks, torch.float32, (N, A, 1))
    row = 0
    if rnn_states is not None:
        _device_tensor(fn, "rnn_states", rnn_states, torch.float32)
        if rnn_states.dim() < 3 or tuple(rnn_states.shape[:2]) != (N, A):
            raise ValueError("eval_step: rnn_states must be [N, A, R, H], not %s" % (tuple(rnn_states.shape),))
        row = rnn_states.numel() // (N * A)
    for name, t in (("done", done), ("sums", sums), ("masks", masks), ("rnn_states", rnn_states)):
        if t is not None and t.device != reward.device:
            raise ValueError("eval_step: %s is on %s and reward on %s" % (name, t.device, reward.device))
    plan = _lib.GmpeEvalStepPlan(N, A, row, int(bool(first)), reward.data_ptr(), done.data_ptr(), sums.data_ptr(), masks.data_ptr(),
                                 None if rnn_states is None else rnn_states.data_ptr())
    _lib.check(_lib.load().gmpe_eval_step(reward.device.index, C.byref(plan), _stream(reward.device)), "gmpe_eval_step")


def eval_mean(values, out=None):
    """np.mean of a contiguous float64 device tensor (any shape, read flat) as a 0-dim float64 device tensor, bit for bit NumPy's: log_env's mean of
    eval_average_episode_rewards (graph_mpe_runner.py:512-516). One launch (gmpe_eval_mean) on the current stream."""
    fn = "eval_mean"
    _device_tensor(fn, "values", values, torch.float64)
    if values.numel() < 1:
        raise ValueError("eval_mean: values is empty")
    if out is None:
        out = torch.empty((), dtype=torch.float64, device=values.device)
    else:
        _device_tensor(fn, "out", out, torch.float64, ())
    plan = _lib.GmpeEvalMeanPlan(values.numel(), values.data_ptr(), out.data_ptr())
    _lib.check(_lib.load().gmpe_eval_mean(values.device.index, C.byref(plan), _stream(values.device)), "gmpe_eval_mean")
    return out
