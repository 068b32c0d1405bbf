"""The exchange of a data-parallel learner's batch statistics (include/gmpe.h gmpe_compute_returns_shard, gmpe_ppo_loss_shard).

Every rank keeps its DeviceRolloutBuffer where its rollout was produced and only gradients cross ranks (clip_and_step(..., shards=x) gathers and sums
them through the same object: see optim.py). The three reductions of the learner path that are over "the batch" — the mean / std of the advantages, ValueNorm.update's batch means, the denominators of the loss means — run in two phases:
LOCAL leaves a few doubles per shard (`local`: f64 [3] or [4] on the device), the caller gathers them into `all` ([world, k], rank order = row order),
APPLY merges the rows in index order. The result is the statistic of the whole batch, the same bits on every shard.

`shards=` of compute_returns / normalized_advantages / ppo_losses takes any object with

    exchange(local) -> [world, k]    the gathered tensor, same dtype and device as `local`, row r = rank r's `local`
    world, rank                      ints

ProcessGroupExchange is the one over torch.distributed:

    x = gmpe.learner_shards.ProcessGroupExchange()          # the default process group
    advantages = buf.normalized_advantages(shards=x)
    res = gmpe.ppo_losses(logits, values, sample, args, value_normalizer, shards=x, reduce="mean")

Limits: each rank draws its minibatches from its own buffer with its own permutation (a globally shared permutation is not built), and the cost of the
extra launch and of the 24 / 32-byte collective per call has not been measured."""
import torch

MAX_WORLD = 4096


class ProcessGroupExchange(object):
    """all_gather_into_tensor of `local` over a torch.distributed process group (None: the default group). Rank order is row order."""

    def __init__(self, group=None):
        import torch.distributed as dist
        if not dist.is_available() or not dist.is_initialized():
            raise RuntimeError("ProcessGroupExchange needs an initialised torch.distributed process group")
        self.group = group
        self.world, self.rank = int(dist.get_world_size(group)), int(dist.get_rank(group))

    def exchange(self, local):
        import torch.distributed as dist
        local = local.contiguous()
        out = torch.empty((self.world,) + tuple(local.shape), dtype=local.dtype, device=local.device)
        dist.all_gather_into_tensor(out, local.unsqueeze(0), group=self.group)     # [1, k] pieces of [world, k]: the form every backend takes
        return out


def check_shards(shards):
    """-> world of a `shards=` argument, or TypeError / ValueError."""
    if not callable(getattr(shards, "exchange", None)) or not hasattr(shards, "world") or not hasattr(shards, "rank"):
        raise TypeError("shards must have exchange(local), world and rank (gmpe.learner_shards.ProcessGroupExchange)")
    world, rank = int(shards.world), int(shards.rank)
    if not 1 <= world <= MAX_WORLD or not 0 <= rank < world:
        raise ValueError("shards.world must be in 1 .. %d and shards.rank in 0 .. world - 1 (got world %d, rank %d)" % (MAX_WORLD, world, rank))
    return world


def check_all_stats(all_stats, local, what, dtype=torch.float64):
    """all_stats: the gathered [world, k] of `local` [k] -> world. Checked before anything is launched. dtype: float64 for the statistics, float32 for
    clip_and_step's packed gradients."""
    k = int(local.numel())
    if not isinstance(all_stats, torch.Tensor) or all_stats.dim() != 2 or all_stats.shape[1] != k:
        raise ValueError("%s: all_stats must be a tensor of shape (world, %d)" % (what, k))
    if all_stats.dtype != dtype:
        raise ValueError("%s: all_stats must be %s, not %s" % (what, str(dtype).replace("torch.", ""), all_stats.dtype))
    world = int(all_stats.shape[0])
    if not 1 <= world <= MAX_WORLD:
        raise ValueError("%s: world = %d is outside 1 .. %d" % (what, world, MAX_WORLD))
    if all_stats.device != local.device:
        raise ValueError("%s: all_stats must be on %s (the device of .local)" % (what, local.device))
    if not all_stats.is_contiguous():
        raise ValueError("%s: all_stats must be contiguous" % what)
    return world


def gather(shards, local, what, dtype=torch.float64):
    """shards.exchange(local), checked -> all_stats"""
    world = check_shards(shards)
    all_stats = shards.exchange(local)
    if check_all_stats(all_stats, local, what, dtype) != world:
        raise ValueError("%s: shards.exchange returned %d rows, shards.world is %d" % (what, all_stats.shape[0], world))
    return all_stats


# ------------------------------------------------------ the two-phase protocol of compute_returns_begin / _finish and ppo_losses_begin / _finish
# Their handles (engine.ReturnsShard, ppo_loss.PPOLossShard) carry `.plan` (the shard plan), `.local` and `.done`. engine and ppo_loss import this
# module inside their functions and this one imports them inside its own: neither import is at module level.
def _launch(entry, sp, dev):
    import ctypes as C
    from . import _lib
    from .engine import _stream_of
    ordinal = dev.index if dev.index is not None else torch.cuda.current_device()
    _lib.check(getattr(_lib.load(), entry)(ordinal, C.byref(sp), _stream_of(dev)), entry)


def begin(entry, sp, base, k, dev):
    """GMPE_SHARD_LOCAL of the C entry point `entry`: sp, its fresh shard plan, around the checked plan `base` -> `.local`, f64 [k] on dev"""
    from . import _lib
    from .engine import _need_cuda
    _need_cuda(dev)
    sp.base = base
    local = torch.empty((k,), dtype=torch.float64, device=dev)
    sp.phase, sp.world, sp.local = _lib.SHARD_LOCAL, 1, local.data_ptr()
    _launch(entry, sp, dev)
    return local


def finish(entry, handle, dev, all_stats, what, again):
    """GMPE_SHARD_APPLY on a handle of begin, once: `again` is the caller's RuntimeError text for a second call, `what` its name -> world"""
    from . import _lib
    from .engine import _need_cuda
    if handle.done:
        raise RuntimeError(again)
    world = check_all_stats(all_stats, handle.local, what)
    _need_cuda(dev)
    sp = handle.plan
    sp.phase, sp.world, sp.all = _lib.SHARD_APPLY, world, all_stats.data_ptr()
    _launch(entry, sp, dev)
    handle.done = True
    return world
