"""Batched evaluation of a policy: GMPERunner.render(get_metrics=True) (onpolicy/runner/shared/graph_mpe_runner.py:526-1060) over one episode per env.

The reference plays `render_episodes` episodes one after another on one env, builds `process_infos` dicts after each, reduces them through the
base runner's `get_*` helpers (base_runner.py:194-574) and prints / writes the min, 10 %, median, 90 %, max and mean of each metric. Here every env
of the engine plays one episode from `reset()`; the policy stays the caller's. Per step, `record()` is one launch of gmpe_episode_record on the
engine's stream (no host synchronisation): it books the step and writes the masks / stop rows the policy acts with next. `summary()` computes the
per-episode columns and their order statistics on the device and reads them once.

`episodes_per_env=R` plays R episodes per env back to back across the engine's auto-resets, as the reference's `render_episodes` loop does on its one
env: record() is then one launch of gmpe_episode_record_series, every env carries its own episode and step counters, an env that finishes early starts
its next episode at once, and the R * N episodes are summarised together. `merge()` summarises the episodes of several finished evaluators (the shard
engines of a MultiDeviceGraphMPEVecEnv: `shard_evaluators`) as one: the records are merged, not the summaries, so every statistic is the one a single
engine over all the envs gives.

`dt` defaults to the world's dt (engine.cfg.dt): the reference's `self.dt` (base_runner.py:216, 492) is never assigned, so its render loop raises
AttributeError as shipped; the world's dt is what its "Hardcoding `dt`" note means.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

COLUMNS = ["reward", "frac", "success", "collisions", "fairness", "dist_mean", "time_mean", "time_fairness", "stddev_param",
           "time_stddev_param", "total_dists_traveled", "total_time_taken", "conformance", "delta_space", "spacing_violations", "steps"]
STATS = ["min", "p10", "median", "p90", "max", "mean", "std"]
SUCCESS_COLUMN = COLUMNS.index("success")
DEFAULT_MIN_DIST_THRESH = 0.05          # onpolicy/scripts/eval_mpe.py:66
MAX_EPISODES = 2 ** 31 - 1              # gmpe_episode_summary's row limit

# the lines the render loop prints with one number (graph_mpe_runner.py:830-904) -> (column, statistic)
_SIX = ("min", "p10", "median", "p90", "max", "mean")
SUMMARY_LABELS = [("Rewards", "reward", "mean"), ("Frac of episode", "frac", "mean")]
SUMMARY_LABELS += [("Success rates " + s, "success", k) for s, k in (("mean", "mean"), ("median", "median"), ("minimum", "min"),
                                                                      ("0.1 quantile", "p10"), ("0.9 quantile", "p90"), ("maximum", "max"))]
SUMMARY_LABELS += [("Num collisions", "collisions", "mean"), ("Fairness Median", "fairness", "median"), ("Fairness Mean", "fairness", "mean")]
SUMMARY_LABELS += [("Fair %s:" % s, "fairness", k) for s, k in (("Minimum", "min"), ("0_1 Quantile", "p10"), ("Median", "median"),
                                                                 ("0.9 Quantile", "p90"), ("Maximum", "max"))]
SUMMARY_LABELS += [("Stddev %s:" % s, "stddev_param", k) for s, k in (("Minimum", "min"), ("0_1 Quantile", "p10"), ("Median", "median"),
                                                                       ("0.9 Quantile", "p90"), ("Maximum", "max"), ("Mean", "mean"))]
SUMMARY_LABELS += [("Time Fair %s:" % s, "time_fairness", k) for s, k in (("Minimum", "min"), ("0.1 Quantile", "p10"), ("Median", "median"),
                                                                           ("0.9 Quantile", "p90"), ("Maximum", "max"), ("Mean", "mean"))]
for _name, _col in (("Time Stddev", "time_stddev_param"), ("Dist Mean", "dist_mean"), ("Time Mean", "time_mean")):
    SUMMARY_LABELS += [("%s %s:" % (_name, s), _col, k) for s, k in (("Minimum", "min"), ("0.1 Quartile", "p10"), ("Median", "median"),
                                                                      ("0.9 Quartile", "p90"), ("Maximum", "max"), ("Mean", "mean"))]
SUMMARY_LABELS += [("Total Dists Traveled Median:", "total_dists_traveled", "median"), ("Total Time Taken Median:", "total_time_taken", "median"),
                   ("Conformance_percentage Mean:", "conformance", "mean"), ("Conformance_percentage median:", "conformance", "median"),
                   ("Delta_space Mean:", "delta_space", "mean"), ("Delta_space median:", "delta_space", "median"),
                   ("Spacing violations Mean:", "spacing_violations", "mean"), ("Spacing violations median:", "spacing_violations", "median")]

# csv_data of the render loop (graph_mpe_runner.py:976-1040) after its five leading settings: (column, statistic), or a per-agent list
_CSV_STATS = [("frac", "mean")] + [("success", k) for k in _SIX] + [("collisions", "mean"), "rewards", "rewards/A", "rewards/(A*T)", "dists_traveled",
              "time_taken"]
_CSV_STATS += [("conformance", k) for k in ("mean", "median", "std")] + [("delta_space", k) for k in ("mean", "median", "std")]
for _col in ("time_fairness", "time_stddev_param", "dist_mean", "time_mean"):
    _CSV_STATS += [(_col, k) for k in ("mean", "min", "p10", "median", "p90", "max")]
for _col in ("total_dists_traveled", "total_time_taken"):
    _CSV_STATS += [(_col, k) for k in ("median", "mean", "p10", "p90", "min", "max")]
_CSV_STATS += [("fairness", k) for k in ("mean", "min", "p10", "median", "p90", "max")]
_CSV_STATS += [("spacing_violations", k) for k in ("mean", "median", "std")]


def _engine_of(engine):
    """A GmpeEngine, or the engine of a BatchedGraphMPEVecEnv."""
    from .engine import GmpeEngine
    eng = engine if isinstance(engine, GmpeEngine) else getattr(engine, "engine", None)
    if not isinstance(eng, GmpeEngine):
        raise TypeError("engine must be a gmpe GmpeEngine (or a BatchedGraphMPEVecEnv's .engine)")
    return eng


def summary_from_stats(stats, dists_traveled, time_taken, episodes):
    """The summary dict from {column: {statistic: value}} and the per-agent sums (what BatchedEvaluator.summary returns)."""
    out = {lab: stats[c][k] for lab, c, k in SUMMARY_LABELS}
    out["dists_traveled"], out["time_taken"] = np.array(dists_traveled, dtype=np.float64), np.array(time_taken, dtype=np.float64)
    out["stats"] = stats
    out["episodes"] = int(episodes)
    return out


def csv_values(summary, num_agents, episode_length, num_obstacles, world_size):
    """The render loop's csv_data row (graph_mpe_runner.py:976-1040) from a summary; render_episodes = the episodes recorded."""
    st, A, T = summary["stats"], num_agents, episode_length
    rew = st["reward"]["mean"]
    row = [num_obstacles, A, world_size, T, summary["episodes"]]
    for item in _CSV_STATS:
        if isinstance(item, tuple):
            row.append(st[item[0]][item[1]])
        elif item == "rewards":
            row.append(rew)
        elif item == "rewards/A":
            row.append(rew / A)
        elif item == "rewards/(A*T)":
            row.append(rew / (A * T))
        else:
            row.append(np.array(summary[item]))
    return row


class _EpisodeRecords(object):
    """What a BatchedEvaluator and a MergedEvaluation share: complete records steps [R, N] / ret [R, N, A] / final_info [R, N, A, 18] on `device`
    (R = 1 may drop the leading axis) and the metrics, summary and csv row over their R * N episodes. A subclass sets lib, device, R, N, A, T, dt,
    min_dist_thresh, _cfg (the engine config csv_row falls back on) and the three records, calls _alloc_tables(), and says in _check_done() when
    the records are complete."""

    def _alloc_tables(self):
        dev = self.device
        self._episodes = torch.zeros((self.R * self.N, _lib.EVAL_NUM_COLUMNS), dtype=torch.float64, device=dev)
        self._agent_sums = torch.zeros((2, self.A), dtype=torch.float64, device=dev)
        self._stats = torch.zeros((_lib.EVAL_NUM_COLUMNS, _lib.EVAL_NUM_STATS), dtype=torch.float64, device=dev)
        self._last = None

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _check_done(self):
        raise NotImplementedError

    def _metrics(self):
        self._check_done()
        mp = _lib.GmpeEpisodeMetricsPlan()
        mp.num_envs, mp.num_agents, mp.num_steps, mp.dt, mp.min_dist_thresh = self.R * self.N, self.A, self.T, self.dt, self.min_dist_thresh
        mp.steps, mp.ret, mp.final_info, mp.episodes = self.steps.data_ptr(), self.ret.data_ptr(), self.final_info.data_ptr(), self._episodes.data_ptr()
        mp.dists_traveled, mp.time_taken = self._agent_sums[0].data_ptr(), self._agent_sums[1].data_ptr()
        _lib.check(self.lib.gmpe_episode_metrics(self.device.index, C.byref(mp), self._stream()), "gmpe_episode_metrics")

    def episodes(self):
        """(f64 device tensor [episodes_per_env * N, len(COLUMNS)], COLUMNS): one row per episode (row e * N + n: episode e of env n), computed on
        the device; no sync."""
        self._metrics()
        return self._episodes, list(COLUMNS)

    def summary(self):
        """The render loop's summary: a dict keyed by the labels it prints ("Success rates mean", "Fair 0.9 Quantile:", ...), plus
        "dists_traveled" / "time_taken" per agent (its dists_trav_list / time_taken_list) and "stats" {column: {statistic: value}}. One sync."""
        self._metrics()
        sp = _lib.GmpeEpisodeSummaryPlan()
        sp.num_rows, sp.num_columns, sp.success_column, sp.success_agents = self.R * self.N, _lib.EVAL_NUM_COLUMNS, SUCCESS_COLUMN, self.A
        sp.table, sp.out = self._episodes.data_ptr(), self._stats.data_ptr()
        _lib.check(self.lib.gmpe_episode_summary(self.device.index, C.byref(sp), self._stream()), "gmpe_episode_summary")
        host = torch.cat([self._stats.reshape(-1), self._agent_sums.reshape(-1)]).cpu().numpy()
        st = host[:self._stats.numel()].reshape(self._stats.shape)
        sums = host[self._stats.numel():].reshape(2, self.A)
        stats = {c: {k: float(st[i, j]) for j, k in enumerate(STATS)} for i, c in enumerate(COLUMNS)}
        self._last = summary_from_stats(stats, sums[0], sums[1], self.R * self.N)
        return self._last

    def csv_row(self, args=None, summary=None):
        """The values of the render loop's csv_data row (graph_mpe_runner.py:976-1040), in its order; render_episodes = episodes recorded.
        The two per-agent lists stay arrays, as there. `args` supplies num_obstacles / world_size (else the config of the engine, of the first one when merged)."""
        s = summary if summary is not None else (self._last if self._last is not None else self.summary())
        cfg = self._cfg
        g = lambda k, d: getattr(args, k, d) if args is not None else d
        return csv_values(s, self.A, self.T, g("num_obstacles", int(cfg.num_obstacles)), g("world_size", float(cfg.world_size)))


class BatchedEvaluator(_EpisodeRecords):
    """One evaluation episode per env of `engine`, booked on the device.

        ev = BatchedEvaluator(engine, args)
        o = ev.reset()
        for t in range(ev.T):
            o = engine.step(act(o.obs, o.node_obs, o.adj, o.agent_id, ev.masks, ev.available_actions))
            ev.record()
        metrics = ev.summary()

    args: the runner's args (episode_length, min_dist_thresh are read when present); keywords override them. rnn_states: an optional f32 device
    tensor [N, A, R, H] the caller's policy carries: reset() zeroes it, record() zeroes the rows of agents done at the step (graph_mpe_runner.py:628).

    episodes_per_env=R > 1: R episodes per env, back to back across the engine's auto-resets (gmpe_episode_record_series); the loop runs until
    finished(), at most R * T steps. `steps` / `ret` / `final_info` are then [R, N, ...] and episodes() has R * N rows, row e * N + n episode e of
    env n. An episode must end where the engine resets, so episode_length has to be the engine's own (ValueError otherwise)."""

    def __init__(self, engine, args=None, *, episode_length=None, dt=None, min_dist_thresh=None, rnn_states=None, episodes_per_env=1):
        eng = self.engine = _engine_of(engine)
        if eng.out.info is None:
            raise ValueError("the evaluator needs the engine's info output: build the engine with with_info=True")
        self.lib = _lib.load()
        T = episode_length if episode_length is not None else getattr(args, "episode_length", None)
        self.T = int(eng.cfg.episode_length if T is None else T)
        self.dt = float(eng.cfg.dt if dt is None else dt)
        thr = min_dist_thresh if min_dist_thresh is not None else getattr(args, "min_dist_thresh", None)
        self.min_dist_thresh = float(DEFAULT_MIN_DIST_THRESH if thr is None else thr)
        if self.T < 1:
            raise ValueError("episode_length must be >= 1")
        if not (self.dt > 0 and np.isfinite(self.dt)):
            raise ValueError("dt must be finite and > 0")
        N, A, dev = eng.N, eng.A, eng.device
        R = self.R = int(episodes_per_env)
        if R < 1:
            raise ValueError("episodes_per_env must be >= 1")
        if R * N > MAX_EPISODES:
            raise ValueError("episodes_per_env * num_envs = %d is above the summary's limit of 2^31 - 1 rows" % (R * N))
        if R > 1 and self.T != int(eng.cfg.episode_length):
            raise ValueError("episodes_per_env > 1 needs episode_length = %d to be the engine's episode_length = %d: the engine resets an env where "
                             "its own episode ends" % (self.T, int(eng.cfg.episode_length)))
        self.N, self.A, self.device = N, A, dev
        self.n_actions = int(eng.cfg.n_actions)
        if rnn_states is not None:
            if not isinstance(rnn_states, torch.Tensor) or rnn_states.dtype != torch.float32 or not rnn_states.is_contiguous() or \
                    rnn_states.device != dev or rnn_states.dim() < 3 or tuple(rnn_states.shape[:2]) != (N, A):
                raise ValueError("rnn_states must be a contiguous float32 tensor [%d, %d, R, H] on %s" % (N, A, dev))
        self.rnn_states = rnn_states
        self.masks = torch.ones((N, A, 1), dtype=torch.float32, device=dev)
        self.available_actions = torch.ones((N, A, self.n_actions), dtype=torch.float32, device=dev)
        self._cfg = eng.cfg
        self._alloc_tables()
        self._t = None                          # steps recorded since reset(); None before the first reset
        self._finished = False
        self._last = None
        if R == 1:
            self.live = torch.zeros((N,), dtype=torch.uint8, device=dev)
            self.steps = torch.zeros((N,), dtype=torch.int32, device=dev)
            self.ret = torch.zeros((N, A), dtype=torch.float64, device=dev)
            self.final_info = torch.zeros((N, A, _lib.EVAL_INFO_WIDTH), dtype=torch.float32, device=dev)
            rp = self._rec = _lib.GmpeEpisodeRecordPlan()
            rp.live, rp.steps, rp.ret, rp.final_info = self.live.data_ptr(), self.steps.data_ptr(), self.ret.data_ptr(), self.final_info.data_ptr()
        else:
            self.episode = torch.zeros((N,), dtype=torch.int32, device=dev)          # per env: episodes completed, steps of the running one, its returns
            self.t_in_ep = torch.zeros((N,), dtype=torch.int32, device=dev)
            self.ret_running = torch.zeros((N, A), dtype=torch.float64, device=dev)
            self.steps = torch.zeros((R, N), dtype=torch.int32, device=dev)
            self.ret = torch.zeros((R, N, A), dtype=torch.float64, device=dev)
            self.final_info = torch.zeros((R, N, A, _lib.EVAL_INFO_WIDTH), dtype=torch.float32, device=dev)
            rp = self._rec = _lib.GmpeEpisodeSeriesPlan()
            rp.num_episodes = R
            rp.episode, rp.t_in_ep, rp.ret = self.episode.data_ptr(), self.t_in_ep.data_ptr(), self.ret_running.data_ptr()
            rp.steps, rp.ret_out, rp.final_info = self.steps.data_ptr(), self.ret.data_ptr(), self.final_info.data_ptr()
        rp.num_envs, rp.num_agents, rp.num_steps, rp.n_actions = N, A, self.T, self.n_actions
        rp.masks, rp.available_actions = self.masks.data_ptr(), self.available_actions.data_ptr()
        if rnn_states is not None:
            rp.rnn_states, rp.rnn_row = rnn_states.data_ptr(), int(rnn_states[0, 0].numel())

    def reset(self):
        """engine.reset(), records zeroed, masks and available_actions all ones, rnn_states zeroed. Returns the engine's outputs."""
        o = self.engine.reset()
        if self.R == 1:
            self.live.fill_(1)
        else:
            self.episode.zero_()
            self.t_in_ep.zero_()
            self.ret_running.zero_()
        self.steps.zero_()
        self.ret.zero_()
        self.final_info.zero_()
        self.masks.fill_(1.0)
        self.available_actions.fill_(1.0)
        if self.rnn_states is not None:
            self.rnn_states.zero_()
        self._t, self._finished, self._last = 0, False, None
        return o

    def record(self):
        """Book the engine's current outputs as step t (counted here) of every live episode: one launch on the current stream, no sync.
        With episodes_per_env > 1 every env books the step to its own running episode (gmpe_episode_record_series)."""
        if self._t is None:
            raise RuntimeError("record() before reset()")
        o = self.engine.out
        rp = self._rec
        if self.R == 1:
            if self._t >= self.T:
                raise RuntimeError("record() called more than episode_length = %d times since reset()" % self.T)
            rp.t = self._t
            rp.reward, rp.done, rp.info = o.reward.data_ptr(), o.done.data_ptr(), o.info.data_ptr()
            _lib.check(self.lib.gmpe_episode_record(self.device.index, C.byref(rp), self._stream()), "gmpe_episode_record")
        else:
            if self._t >= self.R * self.T:
                raise RuntimeError("record() called more than episodes_per_env * episode_length = %d times since reset()" % (self.R * self.T))
            rp.reward, rp.done, rp.info = o.reward.data_ptr(), o.done.data_ptr(), o.info.data_ptr()
            _lib.check(self.lib.gmpe_episode_record_series(self.device.index, C.byref(rp), self._stream()), "gmpe_episode_record_series")
        self._t += 1

    @property
    def t(self):
        """Steps recorded since reset()."""
        return self._t

    def finished(self):
        """True when every env has played its episodes_per_env episodes (one host synchronisation)."""
        if self._t is None:
            return False
        if not self._finished:
            if self._t == self.R * self.T:
                self._finished = True
            elif self.R == 1:
                self._finished = not bool(self.live.any().item())
            else:
                self._finished = bool((self.episode >= self.R).all().item())
        return self._finished

    def _check_done(self):
        if self._t is None or not (self._t == self.R * self.T or self._finished):
            raise RuntimeError("episodes are complete after %sepisode_length = %d record() calls, or once finished() is True"
                               % ("episodes_per_env * " if self.R > 1 else "", self.R * self.T))


def evaluate(engine, act, args=None, *, stop_when_finished=None, evaluator=None, **kw):
    """Run episodes_per_env (default one) evaluation episodes per env: at most episodes_per_env * T steps of
    act(obs, node_obs, adj, agent_id, masks, available_actions) -> int32 [N, A] device actions, engine.step, record; returns the summary.
    With stop_when_finished=k, every k steps it checks (one sync) whether all envs have finished."""
    ev = evaluator if evaluator is not None else BatchedEvaluator(engine, args, **kw)
    eng = ev.engine
    o = ev.reset()
    k = int(stop_when_finished) if stop_when_finished else 0
    total = ev.R * ev.T
    for t in range(total):
        a = act(o.obs, o.node_obs, o.adj, o.agent_id, ev.masks, ev.available_actions)
        o = eng.step(a)
        ev.record()
        if k and (t + 1) % k == 0 and t + 1 < total and ev.finished():
            break
    return ev.summary()


class MergedEvaluation(_EpisodeRecords):
    """The episodes of several finished evaluators as one record [R, sum of N, ...] on one device (what merge() returns): episodes(), summary() and
    csv_row() with BatchedEvaluator's shapes and keys."""

    def __init__(self, evaluators, device=None):
        evs = list(evaluators)
        if not evs:
            raise ValueError("merge() needs at least one evaluator")
        for ev in evs:
            if not isinstance(ev, BatchedEvaluator):
                raise TypeError("merge() takes BatchedEvaluator objects")
        e0 = evs[0]
        for i, ev in enumerate(evs):
            for k in ("A", "T", "dt", "min_dist_thresh", "R"):
                if getattr(ev, k) != getattr(e0, k):
                    raise ValueError("merge(): evaluator %d has %s = %r, evaluator 0 has %r" % (i, _MERGE_NAMES[k], getattr(ev, k), getattr(e0, k)))
        for i, ev in enumerate(evs):
            if not ev.finished():
                raise RuntimeError("merge(): evaluator %d is not finished (%s of at most %d steps recorded)" % (i, ev.t, ev.R * ev.T))
        N = sum(ev.N for ev in evs)
        if e0.R * N > MAX_EPISODES:
            raise ValueError("merge(): %d episodes are above the summary's limit of 2^31 - 1 rows" % (e0.R * N))
        self.lib = e0.lib
        self.A, self.T, self.dt, self.min_dist_thresh, self.R, self.N = e0.A, e0.T, e0.dt, e0.min_dist_thresh, e0.R, N
        self.device = dev = e0.device if device is None else torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if dev.type != "cuda" or dev.index is None:
            raise ValueError("merge(): device must name one GPU (an ordinal or 'cuda:k')")
        self._cfg = e0.engine.cfg
        R, A = self.R, self.A
        # per episode index, the evaluators' envs in the order given: row e * N + n, as one engine over all the envs lays them out
        self.steps = torch.cat([ev.steps.reshape(R, ev.N).to(dev) for ev in evs], dim=1).contiguous()
        self.ret = torch.cat([ev.ret.reshape(R, ev.N, A).to(dev) for ev in evs], dim=1).contiguous()
        self.final_info = torch.cat([ev.final_info.reshape(R, ev.N, A, _lib.EVAL_INFO_WIDTH).to(dev) for ev in evs], dim=1).contiguous()
        self._alloc_tables()

    def _check_done(self):
        pass                                    # merge() took finished evaluators only


_MERGE_NAMES = {"A": "num_agents", "T": "episode_length", "dt": "dt", "min_dist_thresh": "min_dist_thresh", "R": "episodes_per_env"}


def merge(evaluators, device=None):
    """One summary over the episodes of several finished evaluators with the same num_agents, episode_length, dt, min_dist_thresh and
    episodes_per_env; they may sit on different devices (the shard engines of a MultiDeviceGraphMPEVecEnv). Their steps / ret / final_info records
    are copied to `device` (default: the first evaluator's) and laid out per episode index in the order given — for shards the global env order —
    then gmpe_episode_metrics and gmpe_episode_summary run once on the merged record: every statistic, the order statistics and the fixed-tree
    per-agent sums included, is bit for bit the one a single engine over all the envs gives. Raises ValueError when the parameters differ and
    RuntimeError when an evaluator is unfinished."""
    return MergedEvaluation(evaluators, device)


def shard_evaluators(env, args=None, rnn_states=None, **kw):
    """One BatchedEvaluator per shard engine of a MultiDeviceGraphMPEVecEnv, in shard (global env) order: step every shard's engine with its slice of
    the actions, record() on each, then merge(). rnn_states: None or one tensor per shard, each on its shard's device."""
    engines = getattr(env, "shard_engines", None)
    if not engines:
        raise TypeError("shard_evaluators needs a MultiDeviceGraphMPEVecEnv")
    if rnn_states is not None and len(rnn_states) != len(engines):
        raise ValueError("rnn_states must hold one tensor per shard (%d)" % len(engines))
    return [BatchedEvaluator(e, args, rnn_states=None if rnn_states is None else rnn_states[g], **kw) for g, e in enumerate(engines)]
