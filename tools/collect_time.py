"""What one rollout step with the policy in the loop costs on one MI355X, and what the value head costs, each two ways in one process:

  collect_step  at 4096 envs x 10 agents and at the shipped 64 x 3, recurrent actor and critic (tests/test_gpu_policy.py's mirror modules):
                  new     gmpe.policy.collect_step: get_actions (act_head, value_head writing value_preds[t] in place), the env step, the learner fields
                  parent  the sequence written out from the pieces there were before: the layers, gmpe.action_logits, F.linear for v_out, then
                          DeviceRolloutBuffer.act_step(logits, values, rnn_states=..., rnn_states_critic=...)
                one repetition = one episode of T = 8 steps on a buffer of its own; wall time (perf_counter around the T calls and a synchronize) and
                event time (HIP events around the T calls) per step.
  value_head    gmpe.value_head against F.linear with the shipped v_out: forward at 40 960 and at 192 rows under no_grad, forward + backward at
                512 000 rows (values.backward(g) into features, weight and bias); event time per call.

Three repetitions each, alternating, after one untimed repetition of both paths; every figure of every repetition is written, with its median.

    python tools/collect_time.py [--out profiles/collect_step_time.json]
"""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

T, REPS = 8, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "collect_step_time.json"))
    o = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F
    import gmpe
    import gnn_lib as G
    import head_lib as HL
    from gmpe import policy
    from gmpe.engine import GmpeEngine
    from gmpe.rollout import DeviceRolloutBuffer
    from test_gpu_policy import _Net
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    dev = "cuda:0"
    recs = []

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

    def measure(paths, per, what, **extra):
        for fn in paths.values():
            fn()
        times = {k: [] for k in paths}
        for _ in range(REPS):
            for k, fn in paths.items():
                times[k].append(timed(fn))
        for k in paths:
            wall, event = sorted(w / per for w, _ in times[k]), sorted(e / per for _, e in times[k])
            rec = dict(what=what, path=k, wall_us=[round(x, 1) for x in wall], event_us=[round(x, 1) for x in event], wall_us_median=round(wall[1], 1),
                       event_us_median=round(event[1], 1), repetitions=REPS, calls_per_repetition=per, **extra)
            recs.append(rec)
            print(json.dumps(rec), flush=True)

    # ------------------------------------------------------------------ collect_step against the hand-written sequence
    for N, A in ((4096, 10), (64, 3)):
        cfg = gmpe.make_config(num_envs=N, num_agents=A, episode_length=25, seed=7)
        key = G.ACTOR if int(cfg.node_feats) == 7 else G.ROTATE
        bargs = types.SimpleNamespace(gamma=0.99, gae_lambda=0.95, use_gae=True, use_proper_time_limits=False, use_valuenorm=False, use_popart=False)
        engines = [GmpeEngine(cfg, device=0) for _ in range(2)]
        actor, critic = _Net(key, engines[0].D, "act").to(dev), _Net(key, engines[0].D, "v_out", seed=12).to(dev)
        bufs = [DeviceRolloutBuffer(e, T, use_centralized_V=False, policy_fields="all", learner_fields="all", args=bargs, recurrent_N=1, hidden_size=64)
                for e in engines]
        for b in bufs:
            b.warmup()
        rows = N * A

        def new(b=bufs[0]):
            for _ in range(T):
                policy.collect_step(actor, critic, b)
            b.after_update()

        def parent(b=bufs[1]):
            with torch.no_grad():
                for t in range(T):
                    E = int(b._node_obs.shape[-2])
                    x, adj = b._node_obs[t].reshape(rows, E, -1), b._adj[t].reshape(-1, E, E)
                    ids, masks, obs = b.agent_id[t].reshape(rows), b.masks[t].reshape(rows, 1), b.obs[t].reshape(rows, -1)
                    f, h = gmpe.rnn_layer(gmpe.mlp_base((obs, gmpe.gnn_base(x, adj, ids, actor.gnn_base)), actor.base),
                                          b.rnn_states[t].reshape(rows, 1, 64), masks, actor.rnn)
                    fc, hc = gmpe.rnn_layer(gmpe.mlp_base((obs, gmpe.gnn_base(x, adj, ids, critic.gnn_base)), critic.base),
                                            b.rnn_states_critic[t].reshape(rows, 1, 64), masks, critic.rnn)
                    b.act_step(gmpe.action_logits(f, actor.act), F.linear(fc, critic.v_out.weight, critic.v_out.bias), rnn_states=h, rnn_states_critic=hc)
            b.after_update()
        measure({"new": new, "parent": parent}, T, "collect_step", num_envs=N, num_agents=A, rows=rows, steps_per_repetition=T,
                note="per step; new: policy.collect_step, parent: layers + action_logits + F.linear(v_out) + act_step")
        for e in engines:
            e.check_errors()
            e.close()
        del bufs, engines
        torch.cuda.empty_cache()

    # ------------------------------------------------------------------ value_head against F.linear
    g = HL.golden()
    lin = torch.nn.Linear(64, 1).to(dev)
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(g["critic.v_out.weight"]))
        lin.bias.copy_(torch.from_numpy(g["critic.v_out.bias"]))
    for rows, bwd, iters in ((40960, False, 50), (192, False, 50), (512000, True, 10)):
        rng = np.random.RandomState(rows)
        feat = torch.from_numpy(rng.randn(rows, 64).astype(np.float32)).to(dev)
        if not bwd:
            out = torch.empty((rows, 1), device=dev)

            def new():
                with torch.no_grad():
                    for _ in range(iters):
                        gmpe.value_head(feat, lin, out=out)

            def parent():
                with torch.no_grad():
                    for _ in range(iters):
                        F.linear(feat, lin.weight, lin.bias)
            with torch.no_grad():
                a, b = gmpe.value_head(feat, lin).clone(), F.linear(feat, lin.weight, lin.bias)
            worst = float((a - b).abs().max() / b.abs().max())
            extra = {}
        else:
            feat.requires_grad_(True)
            gv = torch.from_numpy(rng.randn(rows, 1).astype(np.float32)).to(dev)
            ws = torch.empty((gmpe.value_workspace_bytes(rows),), dtype=torch.uint8, device=dev)

            def step(values_of):
                feat.grad = lin.weight.grad = lin.bias.grad = None
                values_of().backward(gv)
                return feat.grad, lin.weight.grad, lin.bias.grad

            def new():
                for _ in range(iters):
                    step(lambda: gmpe.value_head(feat, lin, workspace=ws))

            def parent():
                for _ in range(iters):
                    step(lambda: F.linear(feat, lin.weight, lin.bias))
            a = [x.clone() for x in step(lambda: gmpe.value_head(feat, lin, workspace=ws))]
            b = [x.clone() for x in step(lambda: F.linear(feat, lin.weight, lin.bias))]
            worst = max(float((x - y).abs().max() / max(1e-30, float(y.abs().max()))) for x, y in zip(a, b))
            extra = dict(workspace_bytes=int(ws.numel()))
        assert worst < 1e-3, worst
        measure({"new": new, "parent": parent}, iters, "value_head", rows=rows, backward=bwd, max_rel_diff_new_vs_parent=worst,
                note="per call; new: gmpe.value_head, parent: F.linear%s" % (" + autograd's backward" if bwd else " (a fresh output per call; new writes in place)"), **extra)
    os.makedirs(os.path.dirname(o.out), exist_ok=True)
    with open(o.out, "w") as f:
        json.dump(recs, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
