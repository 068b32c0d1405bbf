"""Golden vectors for the PPO minibatch generators, produced by RUNNING the reference in this container:

    python tests/golden/make_minibatch_fixture.py        # writes tests/golden/minibatch_generators.npz

What runs: the reference's own GraphReplayBuffer.feed_forward_generator, recurrent_generator and naive_recurrent_generator (onpolicy/utils/graph_buffer.py:368-758),
on a GraphReplayBuffer built as make_buffer_fixture.py builds one and filled with seeded synthetic arrays whose shapes are a real config's (July scenario, 3 agents:
obs_dim 19, 6 entities, 8 node features, 25 actions), so that a DeviceRolloutBuffer can hold the same inputs. Every case records its seed, the torch.randperm the
generator draws after torch.manual_seed(seed), and every array it yields. share_obs / share_agent_id are filled as the runner fills them (all agents' obs /
ids with use_centralized_V, graph_mpe_runner.py:408-413), which is what DeviceRolloutBuffer.share_obs defines.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_buffer_fixture as MB  # noqa: E402

N, A, T, E, D, F, NACT, R, H = 4, 3, 7, 6, 19, 8, 25, 2, 8
NAMES = ("share_obs", "obs", "node_obs", "adj", "agent_id", "share_agent_id", "rnn_states", "rnn_states_critic", "actions", "value_preds", "returns", "masks",
         "active_masks", "action_log_probs", "advantages", "available_actions")
# name, generator, kwargs, seed, centralised, with available_actions, with advantages
CASES = (
    ("ff_one", "ff", dict(num_mini_batch=1), 11, True, True, True),
    ("ff_rem", "ff", dict(num_mini_batch=5), 12, False, False, True),            # 84 samples / 5: 4 never sampled
    ("rec_l5", "rec", dict(num_mini_batch=3, data_chunk_length=5), 13, True, True, True),   # T % L = 2, batch % L = 4, 16 chunks / 3: 1 left
    ("rec_l10", "rec", dict(num_mini_batch=2, data_chunk_length=10), 14, False, False, True),  # T % L = 7, batch % L = 4, 8 chunks / 2
)
# (advantages=None is no case: the reference's generators reshape / cast the advantages unconditionally, graph_buffer.py:422, 632)


def inputs(seed=0):
    rng = np.random.RandomState(seed)
    f32 = np.float32
    return dict(
        obs=rng.randn(T + 1, N, A, D).astype(f32),
        node_obs=rng.randn(T + 1, N, A, E, F).astype(f32),
        adj=np.abs(rng.randn(T + 1, N, A, E, E)).astype(f32),                   # a different matrix per agent: the per-agent rows are told apart
        agent_id=rng.randint(0, 1000, (T + 1, N, A, 1)).astype(np.int32),
        masks=(rng.rand(T + 1, N, A, 1) < 0.8).astype(f32),
        active_masks=(rng.rand(T + 1, N, A, 1) < 0.8).astype(f32),
        value_preds=rng.randn(T + 1, N, A, 1).astype(f32),
        returns=rng.randn(T + 1, N, A, 1).astype(f32),
        available_actions=(rng.rand(T + 1, N, A, NACT) < 0.7).astype(f32),
        rnn_states=rng.randn(T + 1, N, A, R, H).astype(f32),
        rnn_states_critic=rng.randn(T + 1, N, A, R, H).astype(f32),
        actions=rng.randint(0, NACT, (T, N, A, 1)).astype(f32),
        action_log_probs=rng.randn(T, N, A, 1).astype(f32),
        advantages=rng.randn(T, N, A, 1).astype(f32),
    )


def make_buffer(inp, centralized, with_avail):
    GraphReplayBuffer, _ = MB.load_reference()
    import gym
    Box, Discrete = gym.spaces.Box, gym.spaces.Discrete
    args = argparse.Namespace(episode_length=T, n_rollout_threads=N, hidden_size=H, recurrent_N=R, gamma=0.99, gae_lambda=0.95, use_gae=True,
                              use_popart=False, use_valuenorm=False, use_proper_time_limits=False, use_centralized_V=centralized)
    sp = lambda shape: Box(-np.inf, np.inf, shape, np.float32)
    buf = GraphReplayBuffer(args, A, sp((D,)), sp((A * D,) if centralized else (D,)), sp((E, F)), sp((1,)), sp((A,) if centralized else (1,)),
                            sp((E, E)), Discrete(NACT))
    for k in ("obs", "node_obs", "adj", "agent_id", "masks", "active_masks", "value_preds", "returns", "available_actions", "rnn_states",
              "rnn_states_critic", "actions", "action_log_probs"):
        dst = getattr(buf, k)
        assert dst.shape == inp[k].shape and dst.dtype == inp[k].dtype, (k, dst.shape, dst.dtype)
        dst[...] = inp[k]
    if centralized:
        buf.share_obs[...] = inp["obs"].reshape(T + 1, N, 1, A * D).repeat(A, 2)
        buf.share_agent_id[...] = inp["agent_id"].reshape(T + 1, N, 1, A).repeat(A, 2)
    else:
        buf.share_obs[...] = inp["obs"]
        buf.share_agent_id[...] = inp["agent_id"]
    if not with_avail:
        buf.available_actions = None
    return buf


def main():
    import torch
    inp = inputs()
    rec = {"in_" + k: v for k, v in inp.items()}
    rec.update(N=N, A=A, T=T, E=E, D=D, F=F, n_actions=NACT, cases=np.array([c[0] for c in CASES]))
    for name, kind, kw, seed, central, avail, with_adv in CASES:
        buf = make_buffer(inp, central, avail)
        adv = inp["advantages"] if with_adv else None
        n = N * T * A if kind == "ff" else N * T * A // kw["data_chunk_length"]
        torch.manual_seed(seed)
        rec[name + "_perm"] = torch.randperm(n).numpy()
        torch.manual_seed(seed)
        gen = buf.feed_forward_generator(adv, **kw) if kind == "ff" else buf.recurrent_generator(adv, **kw)
        batches = list(gen)
        rec.update({name + "_" + k: v for k, v in dict(seed=seed, centralized=central, avail=avail, with_adv=with_adv, num_batches=len(batches),
                                                         recurrent=kind == "rec", num_mini_batch=kw["num_mini_batch"],
                                                         data_chunk_length=kw.get("data_chunk_length", 0)).items()})
        for b, tup in enumerate(batches):
            assert len(tup) == 16
            for k, v in zip(NAMES, tup):
                rec["%s_%d_%s" % (name, b, k)] = np.array([]) if v is None else v
                rec["%s_%d_%s_none" % (name, b, k)] = v is None
        print(name, len(batches), "batches", [tuple(np.shape(t)) for t in batches[0]])
    # the naive generator of the reference fails for any batch > 1: masks are flattened to [T*N*A, 1] (graph_buffer.py:501), then masks[:-1, ind] (:541)
    buf = make_buffer(inp, True, True)
    torch.manual_seed(1)
    try:
        list(buf.naive_recurrent_generator(inp["advantages"], 2))
        raise SystemExit("the reference's naive_recurrent_generator ran")
    except IndexError as e:
        rec["naive_error"] = "IndexError: %s" % e
        print("naive_recurrent_generator:", rec["naive_error"])
    p = os.path.join(HERE, "minibatch_generators.npz")
    np.savez_compressed(p, **rec)
    print(p, os.path.getsize(p))


if __name__ == "__main__":
    main()
