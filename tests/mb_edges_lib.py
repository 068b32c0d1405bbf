"""NumPy restatement of the minibatch edge lists (include/gmpe.h gmpe_minibatch_edges): the row map of tests/minibatch_lib.py (imported, not copied), then
process_adj's rule (onpolicy/algorithms/utils/gnn_new.py:329-358) per graph: mask = (adj < d) & (adj > 0) on fp32, nonzero in (graph, row, col) order, node ids
graph * E + i. tests/test_minibatch_edges_host.py checks it against the reference's own process_adj on the reference's own minibatches
(tests/golden/minibatch_edges.npz); the GPU tests compare the kernels with it. Also the synthetic inputs of the GPU tests, so that the host test can check on the
CPU that they are not degenerate."""
import numpy as np

import minibatch_lib as M


def edge_mask(adj, d, inclusive=False):
    adj = np.asarray(adj, dtype=np.float32)
    d = np.float32(d)
    return ((adj <= d) if inclusive else (adj < d)) & (adj > np.float32(0))


def edges(adj_batch, d, inclusive=False, dtype=np.int64):
    """[B, E, E] f32 -> edge_index [2, n] (dtype), edge_attr [n, 1] f32, per-graph counts [B]"""
    adj = np.asarray(adj_batch, dtype=np.float32)
    B, E, _ = adj.shape
    mask = edge_mask(adj, d, inclusive)
    ei, ea = [], []
    for b0 in range(0, B, 1024):                              # nonzero per graph (row-major order inside a graph), graphs in order
        g, i, j = np.nonzero(mask[b0:b0 + 1024])
        g = g.astype(np.int64) + b0
        ei.append(np.stack([g * E + i, g * E + j]))
        ea.append(adj[g, i, j])
    ei = np.concatenate(ei, axis=1) if ei else np.zeros((2, 0), np.int64)
    ea = np.concatenate(ea) if ea else np.zeros((0,), np.float32)
    return ei.astype(dtype), ea.reshape(-1, 1), mask.reshape(B, -1).sum(1)


def samples(perm, off, rows, T, N, A, L=None):
    """(t, n, a, ok) of the graphs of one minibatch: minibatch_lib's maps; perm None: the identity; ok False for an out-of-range entry (a graph without edges)"""
    n_valid = T * N * A if L is None else T * N * A // L
    p = np.arange(off + rows, dtype=np.int64) if perm is None else np.asarray(perm, dtype=np.int64)
    ent = p[off:off + rows]
    ok = (ent >= 0) & (ent < n_valid)
    safe = p.copy()
    safe[off:off + rows] = np.where(ok, ent, 0)
    if L is None:
        t, n, a = M.ff_samples(safe, off, rows, T, N, A)
    else:
        (t, n, a), _ = M.rec_samples(safe, off, rows, T, N, A, L)
        ok = np.tile(ok, L)                                   # graph r = l * rows + k
    return t, n, a, ok


def adj_batch(adj5, perm, off, rows, T, N, A, L=None):
    """the adj batch of one minibatch from adj [T+1, N, A, E, E]; the graphs of out-of-range entries are zero"""
    t, n, a, ok = samples(perm, off, rows, T, N, A, L)
    out = np.asarray(adj5)[t, n, a].astype(np.float32)
    out[~ok] = 0
    return out


def minibatch_edges(adj5, perm, off, rows, T, N, A, d, L=None, inclusive=False, dtype=np.int64):
    return edges(adj_batch(adj5, perm, off, rows, T, N, A, L), d, inclusive, dtype)


def truncated(ei, ea, cap):
    """what a call with `cap` writes: the first cap edges"""
    return ei[:, :cap], ea[:cap]


# ---------------------------------------------------------------------- synthetic inputs of the GPU tests
SYN_D = 1.0            # the threshold used with them: distances are multiples of 0.25, so entries equal to it exist


def synthetic_adj(T1, N, E, seed, A=None):
    """[T1, N, E, E] (A None: the compact form) or [T1, N, A, E, E] (a different matrix per ego): Chebyshev distances of points on a 0.25 grid in a square of
    side 4 (about a fifth of the pairs closer than SYN_D, many exactly at it); every fifth graph all zero; every third of the others has one masked node."""
    rng = np.random.RandomState(seed)
    lead = (T1, N) if A is None else (T1, N, A)
    B = int(np.prod(lead))
    pos = rng.randint(0, 17, (B, E, 2)) * 0.25
    d = np.abs(pos[:, :, None, :] - pos[:, None, :, :]).max(-1).astype(np.float32)
    idx = np.arange(B)
    d[idx % 5 == 0] = 0
    for b in idx[(idx % 5 != 0) & (idx % 3 == 0)]:
        k = rng.randint(0, E)
        d[b, k, :] = 0
        d[b, :, k] = 0
    return d.reshape(lead + (E, E))


def synthetic_perm(rows, n_valid, seed, extra=0):
    """`rows + extra` entries in [0, n_valid): a permutation's slice when it fits, draws with repeats otherwise"""
    rng = np.random.RandomState(seed)
    n = rows + extra
    return (rng.permutation(n_valid)[:n] if n <= n_valid else rng.randint(0, n_valid, n)).astype(np.int64)


def conditions(batch, d):
    """what makes an (input, threshold) pair able to fail a wrong kernel: share of off-diagonal edges, a graph without edges, a fully masked node, a tie"""
    batch = np.asarray(batch, dtype=np.float32)
    B, E, _ = batch.shape
    off = ~np.eye(E, dtype=bool)
    share = float(edge_mask(batch, d)[:, off].mean()) if E > 1 else 0.0
    counts = edge_mask(batch, d).reshape(B, -1).sum(1)
    masked = ((batch == 0).all(1) & (batch == 0).all(2)).any(1) & (counts > 0) if E > 1 else np.zeros(B, bool)
    ties = int((batch == np.float32(d)).sum())
    return dict(share=share, empty=int((counts == 0).sum()), masked=int(masked.sum()), ties=ties,
                incl_diff=int(edge_mask(batch, d, True).sum() - edge_mask(batch, d, False).sum()))


# the shape sweep of tests/test_gpu_minibatch_edges.py: (T, N, A) of the source, compact form; tests/test_minibatch_edges_host.py checks these inputs on the CPU
SHAPE_E = (2, 3, 20, 33, 44, 64, 65, 128)
SHAPE_ROWS = (1, 63, 64, 65, 1024, 1025, 8192)
SHAPE_TNA = (5, 6, 3)


def shape_case(E, rows, L=None):
    """-> adj [T+1, N, E, E], perm (rows + 7 entries, the minibatch starts at 3), offset; recurrent: entries are chunks"""
    T, N, A = SHAPE_TNA
    n_valid = T * N * A if L is None else T * N * A // L
    return synthetic_adj(T + 1, N, E, seed=1005 + E), synthetic_perm(rows, n_valid, seed=rows + (L or 0), extra=7), 3
