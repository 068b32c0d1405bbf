"""What one PPO update costs per call on one MI355X, eagerly and as a replayed graph, in one process:

  ppo_update    at the shipped 64 envs x 3 agents (one recurrent minibatch: num_mini_batch 1) and at 4096 x 10 with num_mini_batch 32 (32 000 rows, the
                minibatch of profiles/popart_loss_bw.log), T = 25, chunks of 10, recurrent actor and critic (tests/test_gpu_policy.py's mirror modules):
                  eager     gmpe.policy.ppo_update(..., install="in_place")
                  captured  gmpe.policy.CapturedUpdate.update(sample): the copy of the sample, one graph replay, the host-side step counts
  clip_and_step over the shipped actor's tensors, the case of profiles/optim_step_time.json:
                  eager     gmpe.clip_and_step(optimizer, 10.0, parameters=..., workspace=...)
                  captured  one replay of a graph that holds gmpe.optim.ScheduledStep.step(), then advance_host()

Wall time per call: a host clock around `iters` calls that ends in one synchronise. Twin networks start from equal state and are compared bit for bit
after three calls of each path before anything is timed. Alternating rounds after one untimed window of each path; median and range over the rounds.
The comparison is between the two paths of this run; one run on one box: the spread between boxes is not in it.

    python tools/captured_update_time.py [--rounds 7] [--iters 20] [--out profiles/captured_update_time.json]
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

T, CHUNK, MAX_NORM, LR, EPS = 25, 10, 10.0, 5e-4, 1e-5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "captured_update_time.json"))
    o = ap.parse_args()
    import copy
    import torch
    import gmpe
    import gnn_lib as G
    from gmpe import policy
    from gmpe.engine import GmpeEngine
    from gmpe.rollout import DeviceRolloutBuffer
    from test_gpu_policy import OBS, _Net
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    dev = "cuda:0"
    recs = []
    steps_ahead = (o.rounds + 2) * o.iters + 8
    same = lambda a, b: bool((a.detach().view(torch.int32) == b.detach().view(torch.int32)).all())

    def measure(paths, what, **extra):
        for fn in paths.values():                       # one untimed window per path
            for _ in range(o.iters):
                fn()
        torch.cuda.synchronize()
        wall = {k: [] for k in paths}
        for _ in range(o.rounds):
            for k, fn in paths.items():                 # alternating rounds
                t0 = time.perf_counter()
                for _ in range(o.iters):
                    fn()
                torch.cuda.synchronize()
                wall[k].append((time.perf_counter() - t0) * 1e6 / o.iters)
        med = {k: sorted(v)[len(v) // 2] for k, v in wall.items()}
        for k in paths:
            rec = dict(what=what, path=k, wall_us_median=round(med[k], 1), wall_us_min=round(min(wall[k]), 1), wall_us_max=round(max(wall[k]), 1),
                       eager_over_this=round(med["eager"] / med[k], 2), rounds=o.rounds, iters=o.iters, **extra)
            recs.append(rec)
            print(json.dumps(rec), flush=True)

    # ------------------------------------------------------------------ one ppo_update
    for N, A, nmb in ((64, 3, 1), (4096, 10, 32)):
        cfg = gmpe.make_config(num_envs=N, num_agents=A, episode_length=T, seed=7)
        key = G.ACTOR if int(cfg.node_feats) == 7 else G.ROTATE
        eng = GmpeEngine(cfg, device=0)
        bargs = types.SimpleNamespace(gamma=0.99, gae_lambda=0.95, use_gae=True, use_proper_time_limits=False, use_valuenorm=False, use_popart=False)
        buf = DeviceRolloutBuffer(eng, T, use_centralized_V=False, policy_fields="all", learner_fields="all", args=bargs, recurrent_N=1, hidden_size=64)
        buf.warmup()
        g = torch.Generator(device=dev)
        g.manual_seed(11)
        for t in range(T):
            rnn = torch.rand((N * A, 1, 64), generator=g, device=dev) * 2 - 1
            buf.act_step(torch.randn((N * A, int(cfg.n_actions)), generator=g, device=dev), torch.randn((N * A, 1), generator=g, device=dev),
                         rnn_states=rnn, rnn_states_critic=rnn)
        buf.compute_returns(torch.randn((N, A, 1), generator=g, device=dev))
        sample = next(iter(buf.recurrent_generator(buf.normalized_advantages(None), nmb, CHUNK, perm="device")))
        sample = tuple(None if x is None else x.clone() for x in sample)
        rows = int(sample[1].shape[0])
        eng.check_errors()
        eng.close()
        del buf, eng
        torch.cuda.empty_cache()
        args = types.SimpleNamespace(clip_param=0.2, huber_delta=10.0, entropy_coef=0.01, use_policy_active_masks=True, use_value_active_masks=True,
                                     use_clipped_value_loss=True, use_huber_loss=True, use_valuenorm=False, use_popart=False, use_max_grad_norm=True,
                                     max_grad_norm=MAX_NORM, value_loss_coef=1.0)

        def twin():
            actor, critic = _Net(key, sample[1].shape[1], "act").to(dev), _Net(key, sample[1].shape[1], "v_out", seed=12).to(dev)
            adam = lambda net: torch.optim.Adam(net.parameters(), lr=LR, eps=EPS)
            return actor, critic, adam(actor), adam(critic)
        a, b = twin(), twin()
        cap = policy.CapturedUpdate(*b, sample, args, steps_ahead=steps_ahead + 3)
        paths = {"eager": lambda: policy.ppo_update(*a, sample, args, install="in_place"), "captured": lambda: cap.update(sample)}
        for _ in range(3):                              # equal start, three updates each: the same bits before anything is timed
            ua, ub = paths["eager"](), paths["captured"]()
            assert all(same(getattr(ua, k), getattr(ub, k)) for k in ua._fields)
        assert all(same(p, q) for x, y in zip(a[:2], b[:2]) for p, q in zip(x.parameters(), y.parameters()))
        measure(paths, "ppo_update", num_envs=N, num_agents=A, num_mini_batch=nmb, rows=rows, episode_length=T, data_chunk_length=CHUNK,
                note="per update of one minibatch, wall time; eager: policy.ppo_update(install='in_place'), captured: CapturedUpdate.update")
        del a, b, cap, paths
        torch.cuda.empty_cache()

    # ------------------------------------------------------------------ the clip and the step alone
    net = _Net(G.ACTOR, OBS, "act")
    gen = torch.Generator().manual_seed(5)
    grads = [torch.randn(p.shape, generator=gen) * 0.01 for p in net.parameters()]

    def build():
        ps = list(copy.deepcopy(net).to(dev).parameters())
        for p, gr in zip(ps, grads):
            p.grad = gr.to(dev)
        return ps, torch.optim.Adam(ps, lr=LR, eps=EPS)
    (pa, oa), (pb, ob) = build(), build()
    ws = torch.empty((gmpe.optim.workspace_bytes(oa),), dtype=torch.uint8, device=dev)
    sched = gmpe.optim.ScheduledStep(ob, MAX_NORM, parameters=pb, steps_ahead=steps_ahead + 4)
    sched.step()                                        # every kernel loaded before the capture
    sched.advance_host()
    gmpe.clip_and_step(oa, MAX_NORM, parameters=pa, workspace=ws)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sched.step()

    def replay():
        graph.replay()
        sched.advance_host()
    paths = {"eager": lambda: gmpe.clip_and_step(oa, MAX_NORM, parameters=pa, workspace=ws), "captured": replay}
    for _ in range(3):
        paths["eager"]()
        paths["captured"]()
    assert all(same(p, q) for p, q in zip(pa, pb)) and oa.state_dict()["state"][0]["step"] == ob.state_dict()["state"][0]["step"]
    measure(paths, "clip_and_step", network="actor", tensors=len(grads), elements=sum(x.numel() for x in grads),
            note="per call, wall time; eager: gmpe.clip_and_step, captured: a replayed graph of ScheduledStep.step() + advance_host()")
    os.makedirs(os.path.dirname(o.out), exist_ok=True)
    with open(o.out, "w") as f:
        json.dump(recs, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
