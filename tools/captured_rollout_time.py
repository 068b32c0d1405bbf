"""What one episode's rollout with the policy in the loop costs on one MI355X, eagerly and as a replayed graph, in one process:

  rollout   at the shipped 64 envs x 3 agents and at 4096 x 10, T = 25, recurrent actor and critic (tests/test_gpu_policy.py's mirror modules), ValueNorm:
              eager     gmpe.policy.rollout(actor, critic, buffer, value_normalizer): 25 collect_steps and compute, launch by launch through Python
              captured  gmpe.policy.CapturedRollout(actor, critic, buffer, value_normalizer).replay(): the counter's fill, one graph launch

Both paths run on ONE buffer and engine. Before every repetition the engine's state (set_state), every buffer array and the draw counter are put back
to what they were after warmup(), so every repetition of either path plays the same episode; the two paths' stored arrays are compared bit for bit
once before anything is timed. One repetition = one episode: wall time (perf_counter around the call and a synchronise) and event time (HIP events
around the call). The eager path's event time contains the gaps in which the device waits for the host; the replay's is the nearest thing here to
the device time of the sequence. Alternating repetitions after one untimed repetition of each path; every figure of every repetition is written,
with its median, per episode and per step. The node count is that of a second capture of the same sequence through the public calls — T times
collect_step(..., draw_dev=buffer.act_draw_counter()), then compute — into a graph this tool keeps (keep_graph=True) and counts with
hipGraphGetNodes; a capture executes nothing, and the host's counters and the engine's binding are put back after it. The construction time is the
CapturedRollout's, wall, with everything it waits for.
The comparison is between the two paths of this run; one run on one box: the spread between boxes is not in it.

    python tools/captured_rollout_time.py [--reps 5] [--out profiles/captured_rollout_time.json]
"""
import argparse
import json
import os
import sys
import time
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
# run as a script, python puts tools/ first on the path, where profile.py would shadow the standard library's `profile` that torch's optimisers import
sys.path[:] = [p for p in sys.path if os.path.abspath(p or ".") != HERE]
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

T = 25


def graph_nodes(graph):
    """the nodes of a torch.cuda.CUDAGraph built with keep_graph=True (hipGraphGetNodes of the HIP runtime this process has loaded), or None where
    that runtime cannot be asked"""
    import ctypes as C
    try:
        hip = C.CDLL("libamdhip64.so")
        hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
        n = C.c_size_t(0)
        return int(n.value) if hip.hipGraphGetNodes(C.c_void_p(graph.raw_cuda_graph()), None, C.byref(n)) == 0 else None
    except (OSError, AttributeError):
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "captured_rollout_time.json"))
    o = ap.parse_args()
    if o.reps < 3:
        raise SystemExit("--reps: at least three repetitions")
    import torch
    import gmpe
    import gnn_lib as G
    import trainer_lib as TL
    from gmpe import policy
    from gmpe.engine import GmpeEngine
    from gmpe.rollout import DeviceRolloutBuffer
    from test_gpu_policy import _Net
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    dev = "cuda:0"
    recs = []

    class ValueNorm(TL.ValueNorm):
        def running_mean_var(self):                         # valuenorm.py:48-55
            mean = self.running_mean / self.debiasing_term.clamp(min=self.epsilon)
            return mean, (self.running_mean_sq / self.debiasing_term.clamp(min=self.epsilon) - mean ** 2).clamp(min=1e-2)

    def timed(fn):
        """(wall, event) microseconds of one call of fn, which queues work and does not wait"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return (time.perf_counter() - w0) * 1e6, e0.elapsed_time(e1) * 1e3

    for N, A in ((64, 3), (4096, 10)):
        cfg = gmpe.make_config(num_envs=N, num_agents=A, episode_length=T, seed=7)
        key = G.ACTOR if int(cfg.node_feats) == 7 else G.ROTATE
        bargs = types.SimpleNamespace(gamma=0.99, gae_lambda=0.95, use_gae=True, use_proper_time_limits=False, use_valuenorm=True, use_popart=False)
        eng = GmpeEngine(cfg, device=0)
        actor, critic = _Net(key, eng.D, "act").to(dev), _Net(key, eng.D, "v_out", seed=12).to(dev)
        vn = ValueNorm(dev)
        vn.running_mean.fill_(0.3), vn.running_mean_sq.fill_(0.7), vn.debiasing_term.fill_(0.5)
        buf = DeviceRolloutBuffer(eng, T, use_centralized_V=False, policy_fields="all", learner_fields="all", args=bargs, recurrent_N=1, hidden_size=64)
        buf.warmup()
        policy.rollout(actor, critic, buf, vn)               # every kernel loaded, the buffer's scratch created: construction is then the graph's own cost
        buf.warmup()
        buf.act_draw = 0
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        cap = policy.CapturedRollout(actor, critic, buf, vn)
        torch.cuda.synchronize()
        construction_ms = (time.perf_counter() - w0) * 1e3
        counted, bound = torch.cuda.CUDAGraph(keep_graph=True), eng.out
        with torch.cuda.graph(counted):                     # the sequence CapturedRollout captures, through the public calls; nothing runs
            for _ in range(T):
                policy.collect_step(actor, critic, buf, draw_dev=buf.act_draw_counter())
            policy.compute(critic, buf, vn)
        buf.act_draw, buf.step = 0, 0
        eng.rebind(bound)
        nodes = graph_nodes(counted)
        del counted
        state = eng.get_state()
        names, arrays = zip(*policy._buffer_arrays(buf))
        saved = [t.clone() for t in arrays]
        bound = eng.out

        def restore():
            eng.set_state(state)
            for t, v in zip(arrays, saved):
                t.copy_(v)
            buf.act_draw, buf.step = 0, 0
            eng.rebind(bound)

        paths = {"eager": lambda: policy.rollout(actor, critic, buf, vn), "captured": cap.replay}
        # the same episode from the same start: the same bits, before anything is timed (this is the untimed repetition of each path too)
        stored = {}
        for k, fn in paths.items():
            restore()
            fn()
            torch.cuda.synchronize()
            stored[k] = [t.clone() for t in arrays]
        differ = [n for n, x, y in zip(names, stored["eager"], stored["captured"])
                  if n != "buffer._act_draw_dev" and not torch.equal(x.view(torch.uint8), y.view(torch.uint8))]      # the counter is the replay's alone
        assert not differ and float(stored["eager"][names.index("buffer.value_preds")].abs().max()) > 0, "the replay differs in %s" % differ
        del stored
        times = {k: [] for k in paths}
        for _ in range(o.reps):
            for k, fn in paths.items():                     # alternating repetitions
                restore()
                times[k].append(timed(fn))
        eng.check_errors()
        med = lambda xs: sorted(xs)[len(xs) // 2]
        eager_wall = med([w for w, _ in times["eager"]])
        for k in paths:
            wall, event = [w for w, _ in times[k]], [e for _, e in times[k]]
            rec = dict(what="rollout", path=k, num_envs=N, num_agents=A, rows=N * A, episode_length=T,
                       wall_us=[round(x, 1) for x in wall], event_us=[round(x, 1) for x in event],
                       wall_us_median=round(med(wall), 1), event_us_median=round(med(event), 1),
                       wall_us_per_step_median=round(med(wall) / T, 1), event_us_per_step_median=round(med(event) / T, 1),
                       eager_wall_over_this_wall=round(eager_wall / med(wall), 2), repetitions=o.reps,
                       note="per episode of T steps and compute, every repetition from the same restored state; eager: policy.rollout, captured: "
                            "CapturedRollout.replay")
            if k == "captured":
                rec.update(graph_nodes=nodes, construction_ms=round(construction_ms, 1))
            recs.append(rec)
            print(json.dumps(rec), flush=True)
        eng.close()
        del cap, buf, eng, arrays, saved, paths
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(o.out), exist_ok=True)
    with open(o.out, "w") as f:
        json.dump(recs, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
