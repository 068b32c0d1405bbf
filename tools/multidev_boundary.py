"""The NumPy boundary of the drop-in vec env as the unchanged runner drives it, over one handle and over MultiDeviceGraphMPEVecEnv.

Per step: float64 one-hot actions [N, A, n_act] in (graph_mpe_runner.py:375-377), the 7-tuple out, the last row of every returned array read. For every
workload it runs one handle on the first device of the first list, then the multi-device class over every `--devices` list, all in ONE process (the GPUs
are opened once). One JSON line per run: env-steps/s, ms per step (median; step_async and step_wait medians apart), G, the device list, and
host_cpus_used = process CPU time / wall time over the timed steps. A list with a repeated ordinal only rehearses the code path on fewer GPUs than shards
("rehearsal": true); only G >= 2 distinct devices says anything about scaling.

step_async queues every shard's launch and its D2H copies into the shared pinned arrays without waiting, so if those copies are really asynchronous its
median stays a small part of the step and the copy time shows up in step_wait.

    python tools/multidev_boundary.py --devices 0,0 [--devices 0,1 --devices 0,1,2,3,4,5,6,7] [--workloads c2,c3] [--steps 40] [--warmup 5]"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from gmpe.vec_env import BatchedGraphMPEVecEnv, MultiDeviceGraphMPEVecEnv  # noqa: E402


def runner_args(wl, n_envs):
    return argparse.Namespace(env_name="GraphMPE", scenario_name=wl["scenario_name"], dynamics_type=None, world_size=wl["world_size"],
                              num_agents=wl["num_agents"], num_landmarks=wl["num_agents"], num_scripted_agents=0, num_obstacles=wl["num_obstacles"],
                              num_walls=wl["num_walls"], collaborative=False, max_speed=2, collision_rew=5, formation_rew=1, goal_rew=5,
                              episode_length=wl["episode_length"], n_rollout_threads=n_envs, total_actions=5, graph_feat_type="relative",
                              discrete_action=True, use_safety_filter=False, seed=1234)


def time_boundary(env, n_envs, n_agents, steps, warmup):
    rng = np.random.RandomState(0)
    n_act = env.action_space[0].n
    onehot = np.eye(n_act)[rng.randint(0, n_act, (4, n_envs, n_agents))]
    env.reset()
    sink = 0.0
    for k in range(warmup):
        env.step(onehot[k % 4])
    t_async, t_wait, t_step = [], [], []
    c0, w0 = time.process_time(), time.perf_counter()
    for k in range(steps):
        t0 = time.perf_counter()
        env.step_async(onehot[k % 4])
        t1 = time.perf_counter()
        out = env.step_wait()
        for x in out[:6]:
            sink += float(x[-1].ravel()[-1])                 # touch every array where the last shard wrote
        t2 = time.perf_counter()
        t_async.append(t1 - t0); t_wait.append(t2 - t1); t_step.append(t2 - t0)
    cpu, wall = time.process_time() - c0, time.perf_counter() - w0
    med = lambda v: sorted(v)[len(v) // 2] * 1e3
    return dict(env_steps_per_s=n_envs / (med(t_step) / 1e3), ms_per_step=med(t_step), mean_ms_per_step=sum(t_step) / steps * 1e3,
                max_ms=max(t_step) * 1e3, step_async_ms=med(t_async), step_wait_ms=med(t_wait), host_cpus_used=round(cpu / wall, 2),
                steps=steps, finite=bool(np.isfinite(sink)))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--devices", action="append", default=None, help="comma-separated device ordinals; repeat for several runs (default 0,0)")
    ap.add_argument("--workloads", default="c2,c3")
    ap.add_argument("--envs", type=int, default=None, help="N over all devices (default: the workload's, 4096)")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    o = ap.parse_args(argv)
    lists = [[int(d) for d in s.split(",")] for s in (o.devices or ["0,0"])]
    seen, usable, _ = bench.host_cpu_budget()
    torch.set_num_threads(max(1, min(16, usable)))
    visible = torch.cuda.device_count()
    for name in o.workloads.split(","):
        wl = bench.WORKLOADS[name]
        N, A = o.envs or wl["envs"], wl["num_agents"]
        args = runner_args(wl, N)
        runs = [("BatchedGraphMPEVecEnv", [lists[0][0]])] + [("MultiDeviceGraphMPEVecEnv", d) for d in lists]
        for cls, devs in runs:
            if cls == "BatchedGraphMPEVecEnv":
                env = BatchedGraphMPEVecEnv(args, num_envs=N, device=devs[0])
            else:
                env = MultiDeviceGraphMPEVecEnv(args, devs, num_envs=N)
            try:
                r = time_boundary(env, N, A, o.steps, o.warmup)
                # the arrays the D2H copies write: the class's own set, or the last shard's row views of the shared [N, ...] arrays
                dst = env._host[0]["obs"] if cls == "BatchedGraphMPEVecEnv" else env._shards[-1]._host[0]["obs"]
                pinned = dst.is_pinned()
            finally:
                env.close()
            line = dict(tool="multidev_boundary", workload=name, envs=N, agents=A, cls=cls, G=len(devs), devices=devs,
                        rehearsal=len(set(devs)) < len(devs), gpus_visible=visible, host_arrays_pinned=bool(pinned),
                        host_threads=torch.get_num_threads(), host_cpus_visible=seen)
            line.update(r)
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
