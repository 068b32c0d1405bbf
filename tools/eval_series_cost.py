"""Cost of the series record (gmpe_episode_record_series, episodes_per_env = 4) next to the one-episode record (gmpe_episode_record, the
unchanged code path) at the bench shapes c2, c3 and c4: both in one process, in alternating rounds, CUDA events; medians and ranges over the
rounds. Then, as counts and not timings, the env steps run per recorded episode for the engine-driven test scenarios under a goal-seeking
policy: one evaluation with episodes_per_env = 4 against four evaluations of one episode per env. Diagnostic.

    python tools/eval_series_cost.py [--reps 200] [--rounds 9]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gmpe  # noqa: E402
from gmpe import evaluate as EV  # noqa: E402
from gmpe.engine import GmpeEngine  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import eval_series_lib as SL  # noqa: E402  (the scenarios and the action rule of the engine-driven tests: one copy)

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


def spread(xs):
    return dict(median=round(statistics.median(xs), 2), min=round(min(xs), 2), max=round(max(xs), 2))


def seek(obs, node_obs, adj, agent_id, masks, available_actions):
    """The engine-driven tests' own goal seeker (tests/eval_series_lib.seek_actions, NumPy on the host: these runs are counted, not timed)."""
    a = SL.seek_actions(obs.cpu().numpy(), available_actions.shape[-1])
    return torch.from_numpy(a).to(obs.device)


def steps_per_episode(kw, N, R):
    """(env steps per recorded episode with episodes_per_env = R, with R evaluations of one episode per env), each loop stopped at the first
    step after which every env has finished."""
    eng = GmpeEngine(gmpe.make_config(num_envs=N, **kw), 0)
    ev = EV.BatchedEvaluator(eng, episodes_per_env=R)
    EV.evaluate(eng, seek, evaluator=ev, stop_when_finished=1)
    series = ev.t * N / float(R * N)
    calls = 0
    one = EV.BatchedEvaluator(eng)
    for _ in range(R):
        EV.evaluate(eng, seek, evaluator=one, stop_when_finished=1)
        calls += one.t
    mean_len = float(ev.steps.double().mean().item())
    eng.close()
    return dict(envs=N, episodes=R * N, series_steps_per_episode=round(series, 3), single_steps_per_episode=round(calls * N / float(R * N), 3),
                mean_episode_length=round(mean_len, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "rounds": a.rounds}
    for key, kw in SHAPES.items():
        T = 25
        eng = GmpeEngine(gmpe.make_config(episode_length=T, seed=3, **kw), 0)
        old, new = EV.BatchedEvaluator(eng), EV.BatchedEvaluator(eng, episodes_per_env=4)
        act = torch.randint(0, eng.cfg.n_actions, (eng.N, eng.A), dtype=torch.int32, device=eng.device)
        old.reset()
        new.reset()
        eng.step(act)

        def rec_old():
            if old.t == old.T:
                old._t = 0                      # the launch itself: same arguments as step t of a fresh episode
            old.record()

        def rec_new():
            if new.t == new.R * new.T:
                new._t = 0
            new.record()

        # both in steady state with every env frozen (the one-episode record is measured so in tools/eval_cost.py), and both live. A live
        # call is two launches: the fill that revives the envs, then the record. The fill is also timed alone (fill_us, zero_us) and
        # *_net_us is the median of the pair less the median of its fill.
        res = {}
        for state in ("frozen", "live"):
            t_old, t_new, f_old, f_new = [], [], [], []
            for _ in range(a.rounds):
                if state == "frozen":
                    old.live.zero_()
                    new.episode.fill_(new.R)
                    t_old.append(timed(rec_old, a.reps))
                    t_new.append(timed(rec_new, a.reps))
                else:
                    t_old.append(timed(lambda: (old.live.fill_(1), rec_old()), a.reps))
                    t_new.append(timed(lambda: (new.episode.zero_(), rec_new()), a.reps))
                    f_old.append(timed(lambda: old.live.fill_(1), a.reps))
                    f_new.append(timed(lambda: new.episode.zero_(), a.reps))
            res[state] = dict(record_us=spread(t_old), series_us=spread(t_new))
            if state == "live":
                res[state].update(fill_us=spread(f_old), zero_us=spread(f_new),
                                  record_net_us=round(statistics.median(t_old) - statistics.median(f_old), 2),
                                  series_net_us=round(statistics.median(t_new) - statistics.median(f_new), 2))
        out[key] = dict(envs=eng.N, agents=eng.A, **res)
        eng.close()
    for name, kw in SL.ENGINE_SCENARIOS.items():
        out["steps_" + name] = steps_per_episode(kw, SL.ENGINE_ENVS, 4)
        out["steps_" + name + "_4096"] = steps_per_episode(kw, 4096, 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
