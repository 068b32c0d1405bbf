"""Golden vectors for the edge lists of PPO minibatches, produced by RUNNING the reference in this container:

    python tests/golden/make_minibatch_edges_fixture.py        # writes tests/golden/minibatch_edges.npz

What runs: the reference's own GraphReplayBuffer.feed_forward_generator / recurrent_generator (onpolicy/utils/graph_buffer.py:368-758) on the seeded buffer of
make_minibatch_fixture.py (same shapes and generator arguments), and then the reference's own TransformerConvNet.process_adj
(onpolicy/algorithms/utils/gnn_new.py:329-358) on every adj_batch they yield, with two values of max_edge_dist. Recorded: the buffer's adj, each case's permutation
and sampler sizes, and per (case, minibatch, threshold) edge_index, edge_attr and the edge count.

The buffer's adj [T+1, N, A, E, E] (E = 6, A = 3, the July scenario's shapes):
  envs 0, 1: real distance matrices, the `ret_adj` a reference rollout returned (tests/golden/july_A3_s2_guided.npz), steps with masked (all-zero) rows and
             columns next to steps without; the A ego copies are the same matrix, as the reference's are;
  envs 2, 3: synthetic matrices whose distances are multiples of 0.25 (so entries EQUAL to a threshold exist), a different matrix per ego (the per-agent copies
             are told apart), some of them all zero (graphs without an edge), some with masked nodes.
gnn_new.py imports torch_geometric, which is not installed here; an inert stub supplies the imported names. process_adj uses none of them.
"""
import os
import sys
import types
import typing

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_minibatch_fixture as MM  # noqa: E402

THRESHOLDS = (1.0, 1.75)
# make_minibatch_fixture.py's cases with seeds of their own: name, generator, kwargs, seed, centralised, with available_actions. The seeds are picked so that every
# minibatch meets what tests/test_minibatch_edges_host.py asserts of an input (a graph without edges, a masked node, a tie, one env-step under two egos).
CASES = (
    ("ff_one", "ff", dict(num_mini_batch=1), 11, True, True),
    ("ff_rem", "ff", dict(num_mini_batch=5), 16, False, False),
    ("rec_l5", "rec", dict(num_mini_batch=3, data_chunk_length=5), 13, True, True),
    ("rec_l10", "rec", dict(num_mini_batch=2, data_chunk_length=10), 15, False, False),
)
ROLLOUT = "july_A3_s2_guided.npz"


def stub_torch_geometric():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    class MessagePassing(object):
        pass

    names = lambda *n: {k: None for k in n}
    nn = mod("torch_geometric.nn", MessagePassing=MessagePassing, **names("TransformerConv", "global_mean_pool", "global_max_pool", "global_add_pool"))
    data = mod("torch_geometric.data", **names("Data", "Batch"))
    loader = mod("torch_geometric.loader", **names("DataLoader"))
    utils = mod("torch_geometric.utils", **names("add_self_loops", "to_dense_batch"))
    typ = mod("torch_geometric.typing", OptPairTensor=typing.Any, Adj=typing.Any, OptTensor=typing.Any, Size=typing.Any)
    mod("torch_geometric", nn=nn, data=data, loader=loader, utils=utils, typing=typ)


def adjacency(seed=5):
    N, A, T, E = MM.N, MM.A, MM.T, MM.E
    g = np.load(os.path.join(HERE, ROLLOUT))
    real = g["ret_adj"].astype(np.float32)
    assert real.shape[1:] == (E, E)
    masked = np.array([bool(((m == 0).all(0) & (m == 0).all(1)).any()) for m in real])
    pick = np.concatenate([np.flatnonzero(masked)[:T + 1], np.flatnonzero(~masked)[:T + 1]])       # 2 envs x (T + 1) slots, masked and unmasked steps alternating
    pick = pick.reshape(2, T + 1).T.reshape(-1)
    adj = np.zeros((T + 1, N, A, E, E), np.float32)
    adj[:, :2] = real[pick].reshape(T + 1, 2, 1, E, E)
    rng = np.random.RandomState(seed)
    for t in range(T + 1):
        for n in (2, 3):
            for a in range(A):
                if n == 3 and (t + a) % 2 == 0:
                    continue                                                                      # all zero: a graph without an edge
                pos = rng.randint(0, 9, (E, 2)) * 0.25                                           # a 2 x 2 square on a 0.25 grid
                d = np.abs(pos[:, None, :] - pos[None, :, :]).max(-1)                            # Chebyshev: every distance a multiple of 0.25
                if (t + a) % 3 == 0:
                    k = rng.randint(0, E)
                    d[k, :] = 0.0
                    d[:, k] = 0.0                                                                 # a masked node
                adj[t, n, a] = d.astype(np.float32)
    return adj


def main():
    import torch
    MM.MB.load_reference()                                   # the stubs of the buffer fixtures (gym, wandb, ...)
    stub_torch_geometric()
    from onpolicy.algorithms.utils.gnn_new import TransformerConvNet
    inp = MM.inputs()
    inp["adj"] = adjacency()
    rec = dict(in_adj=inp["adj"], N=MM.N, A=MM.A, T=MM.T, E=MM.E, thresholds=np.array(THRESHOLDS, np.float64), rollout=ROLLOUT,
               cases=np.array([c[0] for c in CASES]))
    for name, kind, kw, seed, central, avail in CASES:
        buf = MM.make_buffer(inp, central, avail)
        n = MM.N * MM.T * MM.A if kind == "ff" else MM.N * MM.T * MM.A // kw["data_chunk_length"]
        torch.manual_seed(seed)
        rec[name + "_perm"] = torch.randperm(n).numpy()
        torch.manual_seed(seed)
        gen = buf.feed_forward_generator(inp["advantages"], **kw) if kind == "ff" else buf.recurrent_generator(inp["advantages"], **kw)
        batches = list(gen)
        rec.update({name + "_" + k: v for k, v in dict(seed=seed, num_batches=len(batches), recurrent=kind == "rec", num_mini_batch=kw["num_mini_batch"],
                                                         data_chunk_length=kw.get("data_chunk_length", 0)).items()})
        for b, tup in enumerate(batches):
            adj_batch = torch.from_numpy(np.ascontiguousarray(tup[3]))
            rec["%s_%d_graphs" % (name, b)] = adj_batch.shape[0]
            for k, d in enumerate(THRESHOLDS):
                ei, ea = TransformerConvNet.process_adj(adj_batch, d)
                assert ei.dtype == torch.int64 and ei.shape[0] == 2 and ea.shape == (ei.shape[1], 1) and ea.dtype == torch.float32
                rec["%s_%d_d%d_edge_index" % (name, b, k)] = ei.numpy()
                rec["%s_%d_d%d_edge_attr" % (name, b, k)] = ea.numpy()
                rec["%s_%d_d%d_n_edges" % (name, b, k)] = ei.shape[1]
            print(name, b, tuple(adj_batch.shape), [int(rec["%s_%d_d%d_n_edges" % (name, b, k)]) for k in range(len(THRESHOLDS))])
    p = os.path.join(HERE, "minibatch_edges.npz")
    np.savez_compressed(p, **rec)
    print(p, os.path.getsize(p))


if __name__ == "__main__":
    main()
