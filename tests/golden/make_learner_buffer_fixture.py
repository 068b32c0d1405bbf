"""Golden vectors for the learner's fields of the rollout buffer (rnn_states, rnn_states_critic, actions, action_log_probs, value_preds), produced by
RUNNING the reference in this container:

    python tests/golden/make_learner_buffer_fixture.py        # writes tests/golden/learner_buffer_*.npz

What runs: the reference's own `GMPERunner.insert` (onpolicy/runner/shared/graph_mpe_runner.py:384-428 — the RNN rows of done agents zeroed, masks)
driving the reference's own `GraphReplayBuffer.insert` and `after_update` (onpolicy/utils/graph_buffer.py:84-164, 168-283), the runner class used
UNBOUND on a namespace, with the imports and stubs of make_buffer_fixture.py. Inputs are seeded synthetic policy outputs (values, int64 actions,
log-probs, actor and critic RNN states) and dones with single-agent dones and whole-env dones; the env-side arrays are zeros (the learner's fields do
not depend on them). The vectors are data only: the inputs as the runner received them (before its in-place zeroing) and the reference's buffer
contents after T inserts and after after_update.
"""
import argparse
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_buffer_fixture as MB  # noqa: E402

FIELDS = ("rnn_states", "rnn_states_critic", "actions", "action_log_probs", "value_preds")


def learner_fixture(N, A, T, R, H, seed, centralized):
    GraphReplayBuffer, GMPERunner = MB.load_reference()
    import gym
    Box, Discrete = gym.spaces.Box, gym.spaces.Discrete
    D, E, F = 3, 4, 2
    args = argparse.Namespace(episode_length=T, n_rollout_threads=N, hidden_size=H, recurrent_N=R, gamma=0.99, gae_lambda=0.95, use_gae=True,
                              use_popart=False, use_valuenorm=False, use_proper_time_limits=False, use_centralized_V=centralized)
    f32 = np.float32
    sp = lambda shape: Box(-np.inf, np.inf, shape, f32)
    buf = GraphReplayBuffer(args, A, sp((D,)), sp((A * D,) if centralized else (D,)), sp((E, F)), sp((1,)), sp((A,) if centralized else (1,)),
                            sp((E, E)), Discrete(25))
    runner = types.SimpleNamespace(n_rollout_threads=N, num_agents=A, recurrent_N=R, hidden_size=H, use_centralized_V=centralized, buffer=buf)
    rng = np.random.RandomState(seed)
    ids = np.tile(np.arange(A, dtype=np.int64)[None, :, None], (N, 1, 1))
    rec = dict(N=N, A=A, T=T, R=R, H=H, centralized=centralized)
    ins = {k: [] for k in ("values", "actions", "action_log_probs", "rnn_states", "rnn_states_critic", "dones")}
    for t in range(T):
        values = rng.randn(N, A, 1).astype(f32)
        actions = rng.randint(0, 25, (N, A, 1)).astype(np.int64)            # what the policy returns (graph_mpe_runner.py:343-380)
        logp = (-np.abs(rng.randn(N, A, 1)) * 2).astype(f32)
        rnn = rng.randn(N, A, R, H).astype(f32)
        rnn_c = rng.randn(N, A, R, H).astype(f32)
        dones = rng.rand(N, A) < 0.3
        dones[t % N] = True                                     # one env with every agent done per step
        if t % 2:
            dones[(t + 1) % N] = False
        for k, v in zip(ins, (values, actions, logp, rnn, rnn_c, dones)):
            ins[k].append(v.copy())                             # before insert zeroes the done rows in place
        data = (np.zeros((N, A, D), f32), ids, np.zeros((N, A, E, F), f32), np.zeros((N, A, E, E), f32), ids, np.zeros((N, A, 1), f32), dones,
                [{}] * N, values, actions, logp, rnn, rnn_c, None)
        GMPERunner.insert(runner, data)
    for k, v in ins.items():
        rec["in_" + k] = np.array(v)
    for k in FIELDS:
        rec["buf_" + k] = np.array(getattr(buf, k))
    assert buf.step == 0
    buf.after_update()
    for k in FIELDS:
        rec["after_" + k] = np.array(getattr(buf, k))
    return rec


def main():
    for name, kw in (("learner_buffer_R1_H64_central", dict(N=5, A=4, T=5, R=1, H=64, seed=7, centralized=True)),
                     ("learner_buffer_R2_H8_decentral", dict(N=5, A=4, T=5, R=2, H=8, seed=8, centralized=False))):
        d = learner_fixture(**kw)
        p = os.path.join(HERE, name + ".npz")
        np.savez_compressed(p, **d)
        dn = d["in_dones"]
        print(p, os.path.getsize(p), "done agents", int(dn.sum()), "whole-env dones", int(dn.all(-1).sum()),
              "zeroed rnn rows", int((d["buf_rnn_states"][1:] == 0).all(-1).all(-1).sum()), "dtypes", {k: str(d["buf_" + k].dtype) for k in FIELDS})


if __name__ == "__main__":
    main()
