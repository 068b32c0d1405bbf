"""What gmpe_step_tail changes on one MI355X, in one process:

  tail      at 192 lanes (64 x 3) and 40 960 lanes (4096 x 10), n_actions of the engine, R x H = 1 x 64, on a full buffer's arrays:
              one     gmpe.engine.step_tail(...): masks, stop rows, learner fields (and, "counter", the draw counter's advance) in one launch
              pieces  available_actions_from_dones(first = t, count = 1) + engine.masks_from_dones + insert_learner, the three launches it replaces
            "eager": CALLS calls queued from Python between two events, wall and event time per call; "graph": the same CALLS calls captured once
            and replayed, event time per call — the nearest thing here to what a node of a captured rollout costs.
            The fourth launch it replaces, the counter's one-thread launch, has no entry of its own: "counter launch" times
            sample_actions(draw_dev, draw_inc = 1) against the same call with draw_inc = 0, captured and replayed.
  rollout   at 64 x 3 and 4096 x 10, T = 25, recurrent actor and critic (tests/test_gpu_policy.py's mirror modules):
              eager     gmpe.policy.rollout per episode (25 collect_steps and compute), wall
              captured  gmpe.policy.CapturedRollout.replay per episode, wall and event time, with the graph's node count
            every repetition from the same restored state.

Sides alternate inside every repetition, after one untimed repetition; every figure of every repetition is written with its median and its range.
The rollout part uses only calls the commit before gmpe_step_tail has too: run from a checkout of that commit (--only rollout) it measures the
parent, which is how profiles/step_tail_time.json's "parent" records were made, the two checkouts' processes alternating in one session on one box.

    python tools/step_tail_time.py [--reps 7] [--only tail|rollout] [--tag this] [--out profiles/step_tail_time.json] [--append]
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

T, CALLS = 25, 100
SHAPES = ((64, 3), (4096, 10))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", choices=("tail", "rollout"), default=None)
    ap.add_argument("--tag", default="this", help="written into every record: which checkout ran")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "step_tail_time.json"))
    ap.add_argument("--append", action="store_true", help="add the records to the ones --out already holds")
    o = ap.parse_args()
    if o.reps < 3:
        raise SystemExit("--reps: at least three repetitions")
    import torch
    import gmpe
    import gnn_lib as G
    from gmpe import engine as E, policy
    from gmpe.engine import GmpeEngine
    from gmpe.rollout import DeviceRolloutBuffer
    from test_gpu_policy import _Net
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    dev = "cuda:0"
    recs = []
    med = lambda xs: sorted(xs)[len(xs) // 2]

    def emit(**rec):
        for k in [k for k, v in rec.items() if isinstance(v, list) and k.endswith("_us")]:
            xs = rec[k]
            rec[k] = [round(x, 2) for x in xs]
            rec[k + "_median"], rec[k + "_min"], rec[k + "_max"] = round(med(xs), 2), round(min(xs), 2), round(max(xs), 2)
        rec.update(tag=o.tag, repetitions=o.reps)
        recs.append(rec)
        print(json.dumps(rec), flush=True)

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

    def captured(fn):
        """fn's launches as a graph: one untimed run on a side stream, then the capture"""
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        return g

    def alternate(sides):
        """name -> [(wall, event)] over o.reps repetitions, the sides alternating inside each, after one untimed repetition"""
        for fn in sides.values():
            fn()
        torch.cuda.synchronize()
        out = {k: [] for k in sides}
        for _ in range(o.reps):
            for k, fn in sides.items():
                out[k].append(timed(fn))
        return out

    bargs = types.SimpleNamespace(gamma=0.99, gae_lambda=0.95, use_gae=True, use_proper_time_limits=False, use_valuenorm=False, use_popart=False)
    for N, A in SHAPES:
        cfg = gmpe.make_config(num_envs=N, num_agents=A, episode_length=T, seed=7)
        eng = GmpeEngine(cfg, device=0)
        buf = DeviceRolloutBuffer(eng, T, use_centralized_V=False, policy_fields="all", learner_fields="all", args=bargs, recurrent_N=1, hidden_size=64)
        buf.warmup()
        L, K = N * A, int(cfg.n_actions)
        shape = dict(num_envs=N, num_agents=A, rows=L)
        if o.only != "rollout":
            g = torch.Generator(device=dev)
            g.manual_seed(1)
            buf.dones.copy_((torch.rand(buf.dones.shape, generator=g, device=dev) < 0.3).to(torch.uint8))
            ins = dict(values=torch.randn((L, 1), generator=g, device=dev), rnn_states=torch.randn((L, 1, 64), generator=g, device=dev),
                       rnn_states_critic=torch.randn((L, 1, 64), generator=g, device=dev))          # what collect_step hands the tail
            ctr = buf.act_draw_counter()
            t, arrays = 3, buf._learner_arrays()

            def one(counter=False):
                E.step_tail(t, buf.dones, arrays, num_agents=A, masks=buf.masks, active_masks=buf.active_masks, available_actions=buf.available_actions,
                            draw_dev=ctr if counter else None, draw_inc=int(counter), **ins)

            def pieces():
                buf.available_actions_for(t)
                eng.masks_from_dones(buf.dones[t], buf.masks[t + 1], buf.active_masks[t + 1])
                E.insert_learner(t, buf.dones, arrays, **ins)

            loop = lambda fn: (lambda: [fn() for _ in range(CALLS)])
            sides = {"one": loop(one), "one + counter": loop(lambda: one(True)), "pieces": loop(pieces)}
            for k, xs in alternate(sides).items():
                emit(what="tail", mode="eager", side=k, wall_per_call_us=[w / CALLS for w, _ in xs], event_per_call_us=[e / CALLS for _, e in xs],
                     calls=CALLS, note="CALLS calls from Python between two events; 'pieces' is three launches per call", **shape)
            graphs = {k: captured(fn) for k, fn in sides.items()}
            for k, xs in alternate({k: gr.replay for k, gr in graphs.items()}).items():
                emit(what="tail", mode="graph", side=k, event_per_call_us=[e / CALLS for _, e in xs], calls=CALLS,
                     note="the same CALLS calls captured once and replayed: dependent nodes on one stream", **shape)
            from gmpe.act import sample_actions
            logits = torch.randn((L, K), generator=g, device=dev)
            out = buf.act_outputs()
            act = lambda inc: sample_actions(logits, dones_prev=buf.dones[t - 1], stop_action=K // 2, seed=1, num_agents=A, draw=0, draw_dev=ctr,
                                             draw_inc=inc, out=out)
            graphs = {"draw_inc 1": captured(loop(lambda: act(1))), "draw_inc 0": captured(loop(lambda: act(0)))}
            for k, xs in alternate({k: gr.replay for k, gr in graphs.items()}).items():
                emit(what="counter launch", mode="graph", side=k, event_per_call_us=[e / CALLS for _, e in xs], calls=CALLS,
                     note="sample_actions with the device counter, with and without its one-thread launch", **shape)
            del graphs
            buf.warmup()
            buf.act_draw = 0
        if o.only != "tail":
            key = G.ACTOR if int(cfg.node_feats) == 7 else G.ROTATE
            actor, critic = _Net(key, eng.D, "act").to(dev), _Net(key, eng.D, "v_out", seed=12).to(dev)
            policy.rollout(actor, critic, buf)                 # every kernel loaded, the buffer's scratch created
            buf.warmup()
            buf.act_draw = 0
            cap = policy.CapturedRollout(actor, critic, buf)
            state = eng.get_state()
            names, tensors = zip(*policy._buffer_arrays(buf))
            saved = [x.clone() for x in tensors]
            bound = eng.out

            def restore():
                eng.set_state(state)
                for x, v in zip(tensors, saved):
                    x.copy_(v)
                buf.act_draw, buf.step = 0, 0
                eng.rebind(bound)

            def side(fn):
                def run():
                    restore()
                    return timed(fn)
                return run

            sides = {"eager": side(lambda: policy.rollout(actor, critic, buf)), "captured": side(cap.replay)}
            for fn in sides.values():
                fn()
            times = {k: [] for k in sides}
            for _ in range(o.reps):
                for k, fn in sides.items():
                    times[k].append(fn())
            eng.check_errors()
            nodes = None
            try:
                import ctypes as C
                hip = C.CDLL("libamdhip64.so")
                hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
                counted, n = torch.cuda.CUDAGraph(keep_graph=True), C.c_size_t(0)
                with torch.cuda.graph(counted):
                    for _ in range(T):
                        policy.collect_step(actor, critic, buf, draw_dev=buf.act_draw_counter())
                    policy.compute(critic, buf)
                if hip.hipGraphGetNodes(C.c_void_p(counted.raw_cuda_graph()), None, C.byref(n)) == 0:
                    nodes = int(n.value)
                del counted
            except (OSError, AttributeError, TypeError):
                pass
            for k, xs in times.items():
                emit(what="rollout", path=k, episode_length=T, wall_per_episode_us=[w for w, _ in xs], event_per_episode_us=[e for _, e in xs],
                     wall_per_step_us=[w / T for w, _ in xs], graph_nodes=nodes if k == "captured" else None,
                     note="per episode of T collect_steps and compute, every repetition from the same restored state", **shape)
            del cap, tensors, saved
        eng.close()
        del buf, eng
        torch.cuda.empty_cache()
    old = []
    if o.append and os.path.exists(o.out):
        with open(o.out) as f:
            old = json.load(f)
    os.makedirs(os.path.dirname(o.out), exist_ok=True)
    with open(o.out, "w") as f:
        json.dump(old + recs, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
