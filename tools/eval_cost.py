"""Cost of the batched evaluator (gmpe.evaluate) at the bench shapes: gmpe_episode_record per step against the env step it follows, and the
metrics + summary launches (gmpe_episode_metrics, gmpe_episode_summary) at n = 4096 and 65536 episodes. Diagnostic, one process, CUDA events.

    python tools/eval_cost.py [--reps 200]
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gmpe  # noqa: E402
from gmpe import _lib  # noqa: E402
from gmpe import evaluate as EV  # noqa: E402
from gmpe.engine import GmpeEngine  # noqa: E402

SHAPES = {
    "c2": dict(scenario_name="navigation_graph", num_agents=10, num_envs=4096),
    "c3": dict(scenario_name="nav_metered_one_goal_graph_rotate_tube_july", num_agents=10, num_envs=4096),
    "c4": dict(scenario_name="navigation_graph", num_agents=32, num_obstacles=8, num_walls=4, world_size=8.0, num_envs=8192),
}


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps * 1e3          # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0)}
    for key, kw in SHAPES.items():
        T = 25
        eng = GmpeEngine(gmpe.make_config(episode_length=T, seed=3, **kw), 0)
        ev = EV.BatchedEvaluator(eng)
        act = torch.randint(0, eng.cfg.n_actions, (eng.N, eng.A), dtype=torch.int32, device=eng.device)
        ev.reset()
        step_us = timed(lambda: eng.step(act), a.reps)

        def rec():
            if ev.t == ev.T:
                ev._t = 0                       # the launch itself: same arguments as step t of a fresh episode
            ev.record()
        record_us = timed(rec, a.reps)
        ev._t = ev.T
        metrics_us = timed(ev._metrics, 50)
        out[key] = dict(envs=eng.N, agents=eng.A, step_us=round(step_us, 2), record_us=round(record_us, 2),
                        record_over_step=round(record_us / step_us, 4), metrics_us=round(metrics_us, 2))
        eng.close()
    lib = _lib.load()
    for n in (4096, 65536):
        tab = torch.rand((n, _lib.EVAL_NUM_COLUMNS), dtype=torch.float64, device="cuda:0")
        tab[:, EV.SUCCESS_COLUMN] = torch.randint(0, 11, (n,), device="cuda:0").double() / 10
        res = torch.empty((_lib.EVAL_NUM_COLUMNS, _lib.EVAL_NUM_STATS), dtype=torch.float64, device="cuda:0")
        sp = _lib.GmpeEpisodeSummaryPlan()
        sp.num_rows, sp.num_columns, sp.success_column, sp.success_agents = n, _lib.EVAL_NUM_COLUMNS, EV.SUCCESS_COLUMN, 10
        sp.table, sp.out = tab.data_ptr(), res.data_ptr()
        st = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
        us = timed(lambda: _lib.check(lib.gmpe_episode_summary(0, C.byref(sp), st), "gmpe_episode_summary"), 20)
        out["summary_n%d_ms" % n] = round(us / 1e3, 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
