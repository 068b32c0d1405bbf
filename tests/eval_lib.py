"""NumPy restatement of the batched evaluator (include/gmpe.h gmpe_episode_record / _metrics / _summary) — test helper, not a conftest.

Written from the rules, not from the kernels: per-episode columns with 1-D np.mean / np.sum per episode (what the render loop calls), order
statistics with np.percentile / np.median / np.min / np.max, and the success statistics over the flattened [episodes, A] 0/1 matrix.
"""
import numpy as np

COLUMNS = ["reward", "frac", "success", "collisions", "fairness", "dist_mean", "time_mean", "time_fairness", "stddev_param",
           "time_stddev_param", "total_dists_traveled", "total_time_taken", "conformance", "delta_space", "spacing_violations", "steps"]
STATS = ["min", "p10", "median", "p90", "max", "mean", "std"]
KEYS = ["individual_reward", "Dist_to_goal", "Time_req_to_goal", "Num_agent_collisions", "Num_obst_collisions", "Distance_mean",
        "Distance_variance", "Mean_by_variance", "Dists_traveled", "Time_taken", "Time_mean", "Time_stddev", "Time_mean_by_stddev",
        "Conformance", "Delta_spacing", "Spacing_violations", "Min_time_to_goal", "Phase_reached"]
K = {k: i for i, k in enumerate(KEYS)}


def cut_episodes(did_reset, T):
    """The render loop's break rule on a recorded rollout: (first step, length) of each complete episode."""
    s, segs = 0, []
    while True:
        e = next((t for t in range(s, min(s + T, len(did_reset))) if did_reset[t]), s + T - 1)
        if e >= len(did_reset):
            return segs
        segs.append((s, e - s + 1))
        s = e + 1


class Record(object):
    """Per-env record state driven step by step, as gmpe_episode_record defines it."""

    def __init__(self, N, A, T, n_actions=25, width=18, dtype=np.float32):
        self.N, self.A, self.T, self.n_actions = N, A, T, n_actions
        self.live = np.ones(N, bool)
        self.steps = np.zeros(N, np.int32)
        self.ret = np.zeros((N, A), np.float64)
        self.final_info = np.zeros((N, A, width), dtype)
        self.t = 0

    def step(self, reward, done, info):
        """reward [N, A] (the engine's f32, widened), done bool [N, A], info [N, A, W]; returns (masks [N, A, 1], available_actions [N, A, n_actions])."""
        done = np.asarray(done, bool)
        all_done = done.all(axis=1)
        lv = self.live.copy()
        self.ret[lv] = self.ret[lv] + np.asarray(reward)[lv].astype(np.float64)
        fin = lv & (all_done | (self.t == self.T - 1))
        self.final_info[fin] = info[fin]
        self.steps[fin] = self.t + 1
        self.live[fin] = False
        self.t += 1
        masks = np.ones((self.N, self.A, 1), np.float32)
        masks[done] = 0.0
        masks[all_done] = 1.0
        avail = np.ones((self.N, self.A, self.n_actions), np.float32)
        stop = np.zeros(self.n_actions, np.float32)
        stop[self.n_actions // 2] = 1.0
        avail[masks[..., 0] == 0] = stop
        return masks, avail


def episode_columns(final_info, ret, steps, T, dt, min_dist_thresh):
    """f64 [N, len(COLUMNS)] from the records (final_info as recorded, widened to f64)."""
    fi = np.asarray(final_info).astype(np.float64)
    N, A = fi.shape[:2]
    tdt = T * dt
    out = np.zeros((N, len(COLUMNS)))
    for n in range(N):
        f = fi[n]
        ttg = [tdt if v == -1 else v for v in f[:, K["Time_req_to_goal"]].tolist()]
        coll = 0
        for a in range(A):
            coll += f[a, K["Num_agent_collisions"]] / 2.0
            coll += f[a, K["Num_obst_collisions"]]
        last = f[A - 1]
        out[n] = [np.mean(ret[n]), np.max([v / tdt for v in ttg]), np.mean([int(v < min_dist_thresh) for v in f[:, K["Dist_to_goal"]]]), coll,
                  last[K["Mean_by_variance"]], last[K["Distance_mean"]], last[K["Time_mean"]], last[K["Time_mean_by_stddev"]],
                  1.0 / (last[K["Distance_variance"]] + 0.0001), 1.0 / (last[K["Time_stddev"]] + 0.0001), np.sum(f[:, K["Dists_traveled"]].tolist()),
                  np.sum(ttg), np.mean(f[:, K["Conformance"]].tolist()), np.mean(f[:, K["Delta_spacing"]].tolist()),
                  np.mean(f[:, K["Spacing_violations"]].tolist()), steps[n]]
    return out


def agent_sums(final_info, T, dt):
    """The render loop's dists_trav_list / time_taken_list: per-agent sums over the episodes."""
    fi = np.asarray(final_info).astype(np.float64)
    ttg = fi[..., K["Time_req_to_goal"]]
    ttg = np.where(ttg == -1, T * dt, ttg)
    return fi[..., K["Dists_traveled"]].sum(axis=0), ttg.sum(axis=0)


def stats_of(x):
    x = list(np.asarray(x).tolist())
    return {"min": np.min(x), "p10": np.percentile(x, 10), "median": np.median(x), "p90": np.percentile(x, 90), "max": np.max(x),
            "mean": np.mean(x), "std": np.std(x)}


def summary_stats(cols, A):
    """{column: {statistic: value}}; success over the flattened [N, A] 0/1 matrix the render loop keeps (success_rates_arr)."""
    cols = np.asarray(cols)
    out = {c: stats_of(cols[:, i]) for i, c in enumerate(COLUMNS)}
    counts = np.rint(cols[:, COLUMNS.index("success")] * A).astype(np.int64)
    flat = [[1] * int(c) + [0] * int(A - c) for c in counts]
    out["success"] = stats_of(np.array(flat))
    return out
