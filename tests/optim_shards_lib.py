"""What the tests of the sharded gmpe.clip_and_step share (include/gmpe.h gmpe_optim_step_shard): the shapes, the ranks' gradients, the combination rule
restated in numpy, and an in-process exchange that joins replicas running on threads.

The rule: the gradient a sharded call clips and steps is the sum over the ranks of their gradients, a left fold in rank order in float64 that starts at
rank 0's value, rounded to float32 once. Everything after the sum is the existing clip_and_step, so the GPU tests compare with that call on the restated
sum bit for bit and need no tolerance of their own."""
import threading

import numpy as np
import torch

import optim_lib as OL

C = OL.CHUNK
# tensor starts 0, 3, 1027, 2050, 6146, 6147: none but the first is a multiple of 4, and all but the first and the one-element tensor straddle chunks
SIZES = (3, C, C - 1, 64 * 64, 1, C + 1)
SHAPES = tuple((s,) for s in SIZES)
MANY = tuple((1 + i % 5,) for i in range(OL.MAX_TENSORS + 1))          # 65 tensors of one to five elements: two launch groups
WORLDS = (1, 2, 3, 5)
MAX_EXTRA = 16
# rows of three ranks, one element each: BIG tells rank orders apart (1.0 in rank order, 0.0 with the last two swapped), CANCEL leaves rank 2's 0.25 (a
# fold that skips a rank shows), KEEPS is 3.0 in double and 0.0 when added in float32
BIG, SWAPPED, CANCEL, KEEPS = (2.0 ** 60, -2.0 ** 60, 1.0), (2.0 ** 60, 1.0, -2.0 ** 60), (1e8, -1e8 + 3, 0.25), (1e8, 3.0, -1e8)


def fold(rows):
    """rows: the ranks' arrays in rank order -> their sum by the rule"""
    acc = np.asarray(rows[0], np.float32).astype(np.float64)
    for r in rows[1:]:
        acc = acc + np.asarray(r, np.float32).astype(np.float64)
    return acc.astype(np.float32)


def rank_gradients(shapes, world, step, seed=0):
    """[rank][tensor]: optim_lib's gradients, another draw for every rank"""
    return [OL.gradients(shapes, step, seed=seed * 100 + r) for r in range(world)]


def summed(per_rank):
    """[rank][tensor] -> [tensor] by the rule"""
    return [fold([g[i] for g in per_rank]) for i in range(len(per_rank[0]))]


def elems(tensors):
    """gmpe_optim_shard_elems restated. tensors: [(numel, flags, hyper)]"""
    return sum(n for n, _, _ in tensors)


class Lockstep(object):
    """The exchange of `world` replicas that run on threads of one process, on one device and one stream: every replica leaves its `local`, all wait
    at a barrier, every replica stacks the rows in rank order, all wait again before a slot is written anew. The barrier has a timeout and is aborted by a
    replica that fails, so a failure ends the others at once instead of leaving them waiting."""

    def __init__(self, world, timeout=120.0):
        self.world, self.slots, self.barrier, self.calls = world, [None] * world, threading.Barrier(world, timeout=timeout), [0] * world

    def rank(self, r):
        return _Rank(self, r)

    def run(self, fn):
        """fn(rank, shards) on one thread per rank -> the results in rank order; the first failure is raised here"""
        out, errors = [None] * self.world, []

        def body(r):
            try:
                out[r] = fn(r, self.rank(r))
            except BaseException as e:      # noqa: B902  (reported below, on the test's thread)
                errors.append((r, e))
                self.barrier.abort()

        threads = [threading.Thread(target=body, args=(r,)) for r in range(self.world)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        if errors:
            first = [e for e in errors if not isinstance(e[1], threading.BrokenBarrierError)] or errors
            raise first[0][1]
        return out


class _Rank(object):
    def __init__(self, group, rank):
        self.group, self.world, self.rank = group, group.world, rank

    def exchange(self, local):
        g = self.group
        g.slots[self.rank] = local
        g.calls[self.rank] += 1
        g.barrier.wait()
        out = torch.stack(list(g.slots))
        g.barrier.wait()
        return out
