"""Golden vectors for the batched evaluator (gmpe.evaluate), produced by RUNNING the reference in this container:

    python tests/golden/make_eval_fixture.py        # writes tests/golden/eval_metrics.npz

What runs: the reference's own `GMPERunner.render(get_metrics=True)` (onpolicy/runner/shared/graph_mpe_runner.py:526-1060), UNBOUND on a namespace
runner whose `envs` replays a committed guided rollout (tests/golden/*_guided.npz: the recorded rew / done / info rows, `reset_count` = the recorded
auto-reset) and whose policy returns action 0. The render loop itself cuts the rollout into episodes (its break on `reset_count > 0`, or the end of its
`range(episode_length)`), calls the reference's `process_infos` and `get_*` helpers (onpolicy/runner/shared/base_runner.py:194-574) and builds its summary.
The runner carries `dt` = the world's dt: the reference never assigns `self.dt` (only onpolicy/envs/mpe/core.py:125 assigns a `.dt`), so its render loop
raises AttributeError as shipped whenever Time_req_to_goal is recorded.

Recorded per rollout `<name>`:
  <name>/seg        int32 [M, 2]  first recorded step and length of each episode
  <name>/cols       f64 [M, C]    per-episode columns (COLUMNS), from the helpers' outputs with the render loop's reductions
  <name>/success_a  f64 [M, A]    per-agent success (what success_rates_arr holds)
  <name>/dists_trav, time_taken   f64 [A]  the render loop's dists_trav_list / time_taken_list
  <name>/labels, values           the summary lines the render loop prints with one number ("Success rates mean", "Fair 0.9 Quantile:", ...)
  <name>/csv                      f64 [K]  its csv_data row, the two per-agent lists flattened in place (csv_lens gives their lengths)
Data only: the vectors the reference produced, and the inputs they came from stay in the rollout files.
"""
import argparse
import csv as _csv
import io
import os
import sys
import tempfile
import types
from contextlib import redirect_stdout

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_buffer_fixture as MB  # noqa: E402

COLUMNS = ["reward", "frac", "success", "collisions", "fairness", "dist_mean", "time_mean", "time_fairness", "stddev_param",
           "time_stddev_param", "total_dists_traveled", "total_time_taken", "conformance", "delta_space", "spacing_violations", "steps"]
ROLLOUTS = ["july_A3_s2_guided", "july_A6_s4_guided", "julyline_A3_s2_guided", "rotinv_A3_s10_guided", "rotinv_A6_s11_guided", "rotinvglobal_A4_s61_guided",
            "twophase_A3_s23_guided", "twophase_A10_s26_guided", "threephase_A3_s43_guided", "threephasecircle_A5_s94_guided"]
MIN_DIST_THRESH = 0.05      # eval_mpe.py:66
WORLD_DT = 1.0              # world.dt of the air_taxi scenarios (make_world; checked below against a constructed world)


class ReplayEnvs(object):
    """The render loop's `envs`: steps through the recorded rollout with a cursor; reset() does not move it."""

    def __init__(self, d, n_actions):
        self.d, self.cur = d, 0
        self.keys = [str(k) for k in d["info_keys"]]
        self.A = int(d["A"])
        self.action_space = [type("Discrete", (object,), {"n": n_actions})()]      # the render loop dispatches on the class name
        self.starts = []

    def reset(self, *a):
        self.starts.append(self.cur)
        z = np.zeros((1, self.A, 1))
        return z, z, z, z

    def step(self, actions_env):
        d, t = self.d, self.cur
        self.cur += 1
        info = [{k: float(d["info"][t, i, j]) for j, k in enumerate(self.keys)} for i in range(self.A)]
        infos = np.empty((1,), dtype=object)
        infos[0] = info
        z = np.zeros((1, self.A, 1))
        return (z, z, z, z, np.asarray(d["rew"][t], np.float64).reshape(1, self.A, 1), np.asarray(d["done"][t], bool).reshape(1, self.A), infos,
                int(bool(d["did_reset"][t])))


def count_episodes(did_reset, T):
    """Complete episodes under the render loop's break rule that fit in the recording."""
    s, segs = 0, []
    while True:
        e = next((t for t in range(s, min(s + T, len(did_reset))) if did_reset[t]), s + T - 1)
        if e >= len(did_reset):
            return segs
        segs.append((s, e - s + 1))
        s = e + 1


def run(name, GMPERunner):
    import torch
    d = np.load(os.path.join(HERE, name + ".npz"))
    A, T = int(d["A"]), int(d["episode_length"])
    segs = count_episodes(np.asarray(d["did_reset"], bool), T)
    n_actions = 25
    tmp = tempfile.mkdtemp()
    args = argparse.Namespace(render_episodes=len(segs), model_dir=tmp, model_name="m", formation_type="point", world_size=float(d["world_size"]),
                              min_dist_thresh=MIN_DIST_THRESH, episode_length=T, num_agents=A, save_gifs=False, use_render=True)
    policy = types.SimpleNamespace(act=lambda *a, **k: (torch.zeros((A, 1), dtype=torch.int64), torch.zeros((A, 1, 4))))
    envs = ReplayEnvs(d, n_actions)
    runner = types.SimpleNamespace(all_args=args, envs=envs, num_agents=A, episode_length=T, n_rollout_threads=1, recurrent_N=1, hidden_size=4,
                                   num_obstacles=0, dt=WORLD_DT, trainer=types.SimpleNamespace(prep_rollout=lambda: None, policy=policy))
    # the helpers as the render loop calls them, on this runner; process_infos' outputs recorded per episode
    helpers = ["get_fairness_metric", "get_dist_mean", "get_dist_std", "get_time_fairness", "get_time_mean", "get_time_std", "get_dists_traveled",
               "get_time_taken", "get_collisions", "get_fraction_episodes", "get_formation_success", "get_conformation_percentages", "get_delta_spacing",
               "get_spacing_violations"]
    for h in helpers:
        setattr(runner, h, types.MethodType(getattr(GMPERunner, h), runner))
    env_infos = []
    runner.process_infos = lambda infos: env_infos.append(GMPERunner.process_infos(runner, infos)) or env_infos[-1]
    rows = []
    mod = sys.modules[GMPERunner.__module__]
    mod.csv = types.SimpleNamespace(writer=lambda f: types.SimpleNamespace(writerow=lambda r: rows.append(list(r))))
    out = io.StringIO()
    try:
        with redirect_stdout(out):
            GMPERunner.render(runner, get_metrics=True)
    finally:
        mod.csv = _csv
    assert len(env_infos) == len(segs) == len(envs.starts) - 1 and len(rows) == 1, (name, len(env_infos), len(segs))
    assert [s for s, _ in segs] == envs.starts[:-1], (name, segs, envs.starts)
    # per-episode columns: the helpers' outputs reduced as the render loop does (graph_mpe_runner.py:660-718)
    R = runner
    cols, succ = [], []
    dists_tot, time_tot = np.zeros(A), np.zeros(A)
    for (s, n), ei in zip(segs, env_infos):
        frac, success, time_taken = R.get_fraction_episodes(ei)
        frac_max = 1.0 if np.any(frac == 1) else np.max(frac)         # `frac` is a list: the comparison is False, the max is taken
        rew = np.mean(np.sum(np.array([d["rew"][t].reshape(1, A, 1) for t in range(s, s + n)]), axis=0))
        dists = R.get_dists_traveled(ei)
        dists_tot += dists
        time_tot += time_taken
        cols.append([rew, frac_max, np.mean(success), R.get_collisions(ei), R.get_fairness_metric(ei)[-1], R.get_dist_mean(ei)[-1],
                     R.get_time_mean(ei)[-1], R.get_time_fairness(ei)[-1], 1.0 / (R.get_dist_std(ei)[-1] + 0.0001),
                     1.0 / (R.get_time_std(ei)[-1] + 0.0001), np.sum(dists), np.sum(time_taken), np.mean(R.get_conformation_percentages(ei)),
                     np.mean(R.get_delta_spacing(ei)), np.mean(R.get_spacing_violations(ei)), n])
        succ.append(success)
    labels, values = [], []
    for line in out.getvalue().splitlines():
        head, _, last = line.rpartition(" ")
        try:
            v = float(last)
        except ValueError:
            continue
        if head and not head.startswith("num_episodes"):        # the count it prints first is not a metric
            labels.append(head)
            values.append(v)
    row = rows[0]
    flat, lens = [], []
    for v in row:
        a = np.atleast_1d(np.asarray(v, dtype=np.float64))
        flat.extend(a.tolist())
        lens.append(a.size)
    return {"seg": np.array(segs, np.int32), "cols": np.array(cols, np.float64), "success_a": np.array(succ, np.float64),
            "dists_trav": np.array(dists_tot), "time_taken": np.array(time_tot), "labels": np.array(labels), "values": np.array(values, np.float64),
            "csv": np.array(flat, np.float64), "csv_lens": np.array(lens, np.int32), "A": A, "T": T}


def main():
    import ref_harness as H
    _, GMPERunner = MB.load_reference()
    env, sc, w = H.make_july_env(H.july_args(3))
    assert w.dt == WORLD_DT, w.dt
    out = {"columns": np.array(COLUMNS), "rollouts": np.array(ROLLOUTS), "dt": WORLD_DT, "min_dist_thresh": MIN_DIST_THRESH}
    for name in ROLLOUTS:
        r = run(name, GMPERunner)
        print(name, "episodes", len(r["seg"]), "lengths", r["seg"][:, 1].tolist(), "summary lines", len(r["labels"]))
        for k, v in r.items():
            out[name + "/" + k] = v
    p = os.path.join(HERE, "eval_metrics.npz")
    np.savez_compressed(p, **out)
    print(p, os.path.getsize(p))


if __name__ == "__main__":
    sys.exit(main())
