"""NumPy restatement of the minibatch gather (include/gmpe.h gmpe_minibatch_gather): the reference's sampler arithmetic (graph_buffer.py:385-399, 617-622) and
the two index maps from an output row to its sample (t, n, a). tests/test_minibatch_host.py checks it against the reference's own yields
(tests/golden/minibatch_generators.npz); the GPU tests compare the kernel with it."""
import numpy as np

NAMES = ("share_obs", "obs", "node_obs", "adj", "agent_id", "share_agent_id", "rnn_states", "rnn_states_critic", "actions", "value_preds", "returns", "masks",
         "active_masks", "action_log_probs", "advantages", "available_actions")


def ff_sampler(T, N, A, num_mini_batch=None, mini_batch_size=None):
    batch = N * T * A
    if mini_batch_size is None:
        mini_batch_size = batch // num_mini_batch
    return [(i * mini_batch_size, max(0, min(batch, (i + 1) * mini_batch_size) - i * mini_batch_size)) for i in range(num_mini_batch)]


def rec_sampler(T, N, A, num_mini_batch, L):
    chunks = N * T * A // L
    mbc = chunks // num_mini_batch
    return [(i * mbc, mbc) for i in range(num_mini_batch)]


def ff_samples(perm, off, rows, T, N, A):
    """output row r -> j = perm[off + r] over the [T, N, A] flattening"""
    j = np.asarray(perm[off:off + rows], dtype=np.int64)
    return j // (N * A), (j // A) % N, j % A


def rec_samples(perm, off, chunks, T, N, A, L):
    """output row r = l * chunks + k -> f = perm[off + k] * L + l in the [N, A, T] order; and the chunk heads (l = 0)"""
    c = np.asarray(perm[off:off + chunks], dtype=np.int64)
    f = (c[None, :] * L + np.arange(L)[:, None]).reshape(-1)
    dec = lambda f: ((f % T), f // (A * T), (f // T) % A)
    return dec(f), dec(c * L)


def gather(arrays, t, n, a, centralized, heads=None):
    """the 16 arrays of one minibatch from [T+1, N, A, ...] arrays (materialised adjacency) at samples (t, n, a); heads: (t, n, a) of the rnn rows"""
    o = {}
    obs, ids = arrays["obs"], arrays["agent_id"]
    o["share_obs"] = obs[t, n].reshape(len(t), -1) if centralized else obs[t, n, a]
    o["share_agent_id"] = ids[t, n].reshape(len(t), -1) if centralized else ids[t, n, a]
    for k in ("obs", "node_obs", "adj", "agent_id", "actions", "value_preds", "returns", "masks", "active_masks", "action_log_probs", "advantages",
              "available_actions"):
        o[k] = arrays[k][t, n, a] if arrays.get(k) is not None else None
    ht, hn, ha = (t, n, a) if heads is None else heads
    for k in ("rnn_states", "rnn_states_critic"):
        o[k] = arrays[k][ht, hn, ha]
    return o
