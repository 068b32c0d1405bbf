"""Golden vectors for the learner side of a rollout — returns, advantages, stop-action rows — produced by RUNNING the reference in this container:

    python tests/golden/make_returns_fixture.py        # writes tests/golden/returns_advantages.npz and tests/golden/available_actions.npz

What runs (the reference's own code; imports and stubs as in make_buffer_fixture.py):
  * `GraphReplayBuffer.compute_returns` (onpolicy/utils/graph_buffer.py:285-366) for its four branches (use_gae x use_proper_time_limits) with no
    normaliser, with a `ValueNorm` (onpolicy/utils/valuenorm.py) and with a `PopArt` (onpolicy/algorithms/utils/popart.py) whose statistics were
    updated a few times;
  * `GR_MAPPO.train`'s advantage lines (onpolicy/algorithms/graph_mappo.py:294-304), the method called UNBOUND on a namespace whose buffer's
    feed_forward_generator records the `advantages` it is handed and yields nothing; the raw advantages are train's first line on the same objects;
  * `GMPERunner.collect_with_mask` + `get_finished` + `insert` (onpolicy/runner/shared/graph_mpe_runner.py:73-141, 241-335, 384-428), unbound, in the
    order `run()` calls them, with a stub policy that records the available_actions it is given, over two episodes of a fixed dones sequence with
    partly-done envs, fully-done envs and an episode boundary (after_update between them).
Inputs are seeded synthetic arrays; the vectors are data only. The normalisers' statistics are stored as running_mean_var / debiased_mean_var return them,
with the sqrt(var) their denormalize used in this run (a host's torch sqrt may differ from the correctly rounded one by an ulp: tests take it from here).
"""
import argparse
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_buffer_fixture as MB  # noqa: E402

BRANCHES = [(gae, proper) for gae in (True, False) for proper in (False, True)]
NORMS = ("none", "valuenorm", "popart")


def load_reference():
    GraphReplayBuffer, GMPERunner = MB.load_reference()
    # graph_mappo imports the policy class (torch_geometric, absent here); train's advantage lines never touch it
    MB._stub("onpolicy.algorithms.graph_MAPPOPolicy", GR_MAPPOPolicy=object)
    from onpolicy.algorithms.graph_mappo import GR_MAPPO
    from onpolicy.utils.valuenorm import ValueNorm
    from onpolicy.algorithms.utils.popart import PopArt
    return GraphReplayBuffer, GMPERunner, GR_MAPPO, ValueNorm, PopArt


def _buffer(GraphReplayBuffer, N, A, T, n_actions=25, **flags):
    import gym
    Box, Discrete = gym.spaces.Box, gym.spaces.Discrete
    f32 = np.float32
    sp = lambda shape: Box(-np.inf, np.inf, shape, f32)
    args = argparse.Namespace(episode_length=T, n_rollout_threads=N, hidden_size=4, recurrent_N=1, gamma=0.99, gae_lambda=0.95, use_gae=True,
                              use_popart=False, use_valuenorm=False, use_proper_time_limits=False, use_centralized_V=True)
    for k, v in flags.items():
        setattr(args, k, v)
    D, E, F = 4, 4, 3
    return GraphReplayBuffer(args, A, sp((D,)), sp((A * D,)), sp((E, F)), sp((1,)), sp((A,)), sp((E, E)), Discrete(n_actions)), args


def returns_fixture(T=9, N=6, A=4, seed=11):
    import torch
    GraphReplayBuffer, _, GR_MAPPO, ValueNorm, PopArt = load_reference()
    rng = np.random.RandomState(seed)
    torch.manual_seed(seed)
    f32 = np.float32
    rec = dict(T=T, N=N, A=A, gamma=0.99, gae_lambda=0.95)
    rec["rewards"] = rng.randn(T, N, A, 1).astype(f32)
    rec["value_preds"] = (rng.randn(T + 1, N, A, 1) * 0.7).astype(f32)
    rec["masks"] = (rng.rand(T + 1, N, A, 1) > 0.2).astype(f32)
    rec["bad_masks"] = (rng.rand(T + 1, N, A, 1) > 0.25).astype(f32)
    rec["active_masks"] = (rng.rand(T + 1, N, A, 1) > 0.3).astype(f32)
    rec["next_value"] = rng.randn(N, A, 1).astype(f32)
    rec["returns_in"] = (rng.randn(T + 1, N, A, 1) * 3).astype(f32)    # what the buffer held before (slot T survives with GAE)
    norms = {"none": None}
    vn = ValueNorm(1)
    for _ in range(4):
        vn.update(torch.from_numpy((rng.randn(T * N * A, 1) * 2.5 + 1.3).astype(f32)))
    norms["valuenorm"] = vn
    pa = PopArt(8, 1)
    for _ in range(3):
        pa.update(torch.from_numpy((rng.randn(T * N * A, 1) * 1.7 - 0.4).astype(f32)))
    norms["popart"] = pa
    for name, nz in norms.items():
        if nz is not None:
            m, v = nz.running_mean_var() if name == "valuenorm" else nz.debiased_mean_var()
            rec["%s_mean" % name], rec["%s_var" % name] = m.detach().numpy().astype(f32), v.detach().numpy().astype(f32)
            rec["%s_std" % name] = torch.sqrt(v).detach().numpy().astype(f32)     # what denormalize multiplies by in this run (torch's host sqrt)
    for gae, proper in BRANCHES:
        for name, nz in norms.items():
            buf, args = _buffer(GraphReplayBuffer, N, A, T, use_gae=gae, use_proper_time_limits=proper,
                                use_valuenorm=name == "valuenorm", use_popart=name == "popart")
            for k in ("rewards", "value_preds", "masks", "bad_masks", "active_masks"):
                getattr(buf, k)[...] = rec[k]
            buf.returns[...] = rec["returns_in"]
            buf.compute_returns(rec["next_value"].copy(), nz)
            key = "%s_%s_%s" % ("gae" if gae else "mc", "proper" if proper else "plain", name)
            rec["ret_" + key] = buf.returns.copy()
            rec["vp_" + key] = buf.value_preds.copy()
            # GR_MAPPO.train, unbound: its buffer generator records the (normalised) advantages and yields nothing
            seen = []

            def ffg(advantages, num_mini_batch=None, mini_batch_size=None):
                seen.append(np.array(advantages, copy=True))
                return iter(())
            trainer = types.SimpleNamespace(_use_popart=name == "popart", _use_valuenorm=name == "valuenorm", value_normalizer=nz, ppo_epoch=1,
                                            num_mini_batch=1, _use_recurrent_policy=False, _use_naive_recurrent=False, data_chunk_length=10)
            view = types.SimpleNamespace(returns=buf.returns, value_preds=buf.value_preds, active_masks=buf.active_masks, feed_forward_generator=ffg)
            GR_MAPPO.train(trainer, view)
            rec["advn_" + key] = seen[0]
            raw = buf.returns[:-1] - (nz.denormalize(buf.value_preds[:-1]) if nz is not None else buf.value_preds[:-1])   # train's first line
            rec["adv_" + key] = raw
    return rec


def available_actions_fixture(N=5, A=3, T=6, n_actions=25, episodes=2, seed=5):
    import torch
    GraphReplayBuffer, GMPERunner, _, _, _ = load_reference()
    buf, _ = _buffer(GraphReplayBuffer, N, A, T, n_actions=n_actions)
    rng = np.random.RandomState(seed)
    seen = []

    class Policy(object):
        def get_actions(self, *a, available_actions=None, **k):
            seen.append(np.array(available_actions, copy=True))
            M = N * A
            return (torch.zeros(M, 1), torch.zeros(M, 1, dtype=torch.int64), torch.zeros(M, 1), torch.zeros(M, 1, 4), torch.zeros(M, 1, 4))
    import gym
    runner = types.SimpleNamespace(n_rollout_threads=N, num_agents=A, recurrent_N=1, hidden_size=4, use_centralized_V=True, buffer=buf,
                                   all_args=types.SimpleNamespace(num_agents=A), envs=types.SimpleNamespace(action_space=[gym.spaces.Discrete(n_actions)]),
                                   trainer=types.SimpleNamespace(prep_rollout=lambda: None, policy=Policy()))
    runner.get_finished = lambda d: GMPERunner.get_finished(runner, d)
    f32 = np.float32
    all_dones, slots = [], []
    for ep in range(episodes):
        dones_seq = rng.rand(T, N, A) < 0.3
        for t in range(T):
            dones_seq[t, t % N] = True                 # one env with every agent done per step (it auto-resets; its agents still get the stop row next step)
            dones_seq[t, (t + 2) % N] = False
        dones_seq[2] = False                           # a step where no agent anywhere is done (collect_with_mask's flag stays False next step)
        all_dones.append(dones_seq)
        finished = None
        for step in range(T):
            dones = dones_seq[step]
            D, E, F = 4, 4, 3
            obs, node, adj = rng.randn(N, A, D).astype(f32), rng.randn(N, A, E, F).astype(f32), np.abs(rng.randn(N, A, E, E)).astype(f32)
            ids = np.tile(np.arange(A)[None, :, None], (N, 1, 1))
            z = lambda *s: np.zeros(s, f32)
            if step == 0:                              # run(): collect(step) + a row of ones (graph_mpe_runner.py:75-101)
                avail = np.ones((N, A, n_actions), dtype=f32)
                seen.append(avail.copy())
            else:                                      # run(): collect_with_mask with the previous step's `finished` (:103-138)
                active_masks = np.ones((N, A, 1), dtype=np.int32)
                out = GMPERunner.collect_with_mask(runner, step, [], active_masks, finished)
                avail = out[6]
            finished, _ = runner.get_finished(dones)
            data = (obs, ids, node, adj, ids, rng.randn(N, A, 1).astype(f32), dones, [{}] * N, z(N, A, 1), z(N, A, 1), z(N, A, 1),
                    z(N, A, 1, 4), z(N, A, 1, 4), avail)
            GMPERunner.insert(runner, data)
        slots.append(np.array(buf.available_actions, copy=True))
        buf.after_update()
    policy_avail = np.array([np.reshape(a, (N, A, n_actions)) for a in seen]).reshape(episodes, T, N, A, n_actions).astype(f32)
    return dict(N=N, A=A, T=T, n_actions=n_actions, dones=np.array(all_dones), slots=np.array(slots), policy_avail=policy_avail,
                after_update_slot0=np.array(buf.available_actions[0], copy=True))


def main():
    for name, d in (("returns_advantages", returns_fixture()), ("available_actions", available_actions_fixture())):
        p = os.path.join(HERE, name + ".npz")
        np.savez_compressed(p, **d)
        print(p, os.path.getsize(p), sorted(k for k in d if not np.isscalar(d[k]))[:6], "...")


if __name__ == "__main__":
    main()
