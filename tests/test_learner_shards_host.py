"""Host side of the sharded learner statistics (include/gmpe.h gmpe_compute_returns_shard, gmpe_ppo_loss_shard; gmpe.compute_returns_begin / _finish,
gmpe.ppo_losses_begin / _finish, gmpe.learner_shards), no GPU:
(a) the two new plans against the C header, the exported symbols, the ABI version, and the refusals of the C entry points before any device call;
(b) the float64 emulation of the two merge orders (tests/learner_shards_lib.py): pinned to returns_lib.kernel_order_stats shard by shard, inside
    returns_lib.candidate_pairs of the concatenated data for every split, and told from the cheap wrong variants — with which input catches which;
(c) ProcessGroupExchange over gloo at world size 2 (file-store rendezvous): rows arrive in rank order;
(d) every argument error of the two-step wrappers, raised before anything is launched."""
import ctypes as C
import os
import tempfile
import types

import numpy as np
import pytest
import torch

import abi_lib
import gmpe
import learner_shards_lib as LS
import ppo_loss_lib as P
import returns_lib as R
from gmpe import _lib


# ---------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("cname,plan,base", [("gmpe_returns_shard_plan", "GmpeReturnsShardPlan", "GmpeReturnsPlan"),
                                             ("gmpe_ppo_loss_shard_plan", "GmpePpoLossShardPlan", "GmpePpoLossPlan")])
def test_shard_plans_match_the_header(cname, plan, base):
    PP, BP = getattr(_lib, plan), getattr(_lib, base)
    assert abi_lib.c_name(PP) == cname and [f for f, _ in PP._fields_] == ["base", "phase", "world", "local", "all"]
    assert abi_lib.layout(PP) == abi_lib.mirror_layout(PP)
    assert abi_lib.layout(PP)[0] == C.sizeof(BP) + 4 + 4 + 8 + 8                  # the existing plan by value, then the four new fields
    assert abi_lib.layout(BP)[0] == C.sizeof(BP)                                  # the existing plan is untouched
    assert [abi_lib.constant("GMPE_" + k) for k in ("SHARD_LOCAL", "SHARD_APPLY", "SHARD_MAX_WORLD", "RETURNS_SHARD_STATS", "PPO_SHARD_STATS", "ABI_VERSION")] == [
        _lib.SHARD_LOCAL, _lib.SHARD_APPLY, _lib.SHARD_MAX_WORLD, _lib.RETURNS_SHARD_STATS, _lib.PPO_SHARD_STATS, 3]
    assert gmpe.learner_shards.MAX_WORLD == _lib.SHARD_MAX_WORLD


def test_symbols_are_exported_and_the_abi_version_stays():
    assert {"gmpe_compute_returns_shard", "gmpe_ppo_loss_shard"} <= set(_lib.SYMBOLS) & abi_lib.exported()
    assert _lib.load().gmpe_abi_version() == 3 and gmpe.config.ABI_VERSION == 3


def _returns_shard_plan(**over):
    p = _lib.GmpeReturnsShardPlan()
    b = p.base
    b.num_steps, b.flags, b.lanes, b.stride, b.gamma, b.gae_lambda = 4, 1, 10, 10, 0.99, 0.95
    for k in ("rewards", "masks", "value_preds", "returns", "next_value", "advantages", "active_masks", "normalized", "workspace"):
        setattr(b, k, 0x10000)
    b.workspace_bytes = 1 << 20
    p.phase, p.world, p.local, p.all = 0, 2, 0x10000, 0x10000
    for k, v in over.items():
        setattr(b if k.startswith("base_") else p, k[5:] if k.startswith("base_") else k, v)
    return p


def _loss_shard_plan(**over):
    from test_ppo_loss_host import _plan
    p = _lib.GmpePpoLossShardPlan()
    p.base = _plan()
    p.phase, p.world, p.local, p.all = 0, 2, 0x10000, 0x10000
    for k, v in over.items():
        setattr(p.base if k.startswith("base_") else p, k[5:] if k.startswith("base_") else k, v)
    return p


SHARD_BAD = [dict(phase=2), dict(phase=-1), dict(world=0), dict(world=4097), dict(world=-3), dict(phase=0, local=None), dict(phase=0, local=0x10004),
             dict(phase=1, all=None), dict(phase=1, all=0x10004)]


@pytest.mark.parametrize("bad", SHARD_BAD + [dict(base_normalized=None), dict(base_active_masks=None), dict(base_workspace=None), dict(base_workspace_bytes=8),
                                             dict(base_flags=8), dict(base_lanes=0), dict(phase=1, base_returns=None)], ids=lambda b: "-".join(b))
def test_returns_shard_entry_refuses_bad_plans_before_any_device_call(bad):
    lib = _lib.load()
    assert lib.gmpe_compute_returns_shard(0, C.byref(_returns_shard_plan(**bad)), None) == -1
    assert lib.gmpe_last_error().decode().startswith("gmpe_compute_returns_shard:")
    assert lib.gmpe_compute_returns_shard(0, None, None) == -1


@pytest.mark.parametrize("bad", SHARD_BAD + [dict(base_rows=0), dict(base_flags=32), dict(base_out=None), dict(base_workspace=None), dict(base_workspace_bytes=8),
                                             dict(phase=1, base_grad_logits=None), dict(base_flags=16)], ids=lambda b: "-".join(b))
def test_loss_shard_entry_refuses_bad_plans_before_any_device_call(bad):
    lib = _lib.load()
    assert lib.gmpe_ppo_loss_shard(0, C.byref(_loss_shard_plan(**bad)), None) == -1
    assert lib.gmpe_last_error().decode().startswith("gmpe_ppo_loss_shard:")
    assert lib.gmpe_ppo_loss_shard(0, None, None) == -1


def test_the_existing_entry_points_keep_their_error_texts():
    lib = _lib.load()
    p = _returns_shard_plan(base_flags=8).base
    assert lib.gmpe_compute_returns(0, C.byref(p), None) == -1 and lib.gmpe_last_error().decode() == "gmpe_compute_returns: unknown flags"
    q = _loss_shard_plan(base_flags=32).base
    assert lib.gmpe_ppo_loss(0, C.byref(q), None) == -1 and lib.gmpe_last_error().decode() == "gmpe_ppo_loss: unknown flags"


# ---------------------------------------------------------------------------------------------- (b) returns
ALL_RETURNS = LS.RETURNS_CASES + LS.HOST_ONLY_RETURNS_CASES


def _branch_advantages():
    d = R.branch_inputs(LS.BRANCH_T, sum(LS.BRANCH_SPLIT))
    return R.branch_expectations(d, True, False, R.DENORM)[2], d["active_masks"]


def _all_inputs():
    """name -> (adv, active_masks, split) of every sharded returns input of the two test files."""
    out = {n: LS.returns_case(n) for n in ALL_RETURNS}
    adv, am = _branch_advantages()
    out["branch-gae-valuenorm"] = (R._rows(adv), R._rows(am), LS.BRANCH_SPLIT)
    return out


@pytest.mark.parametrize("name", list(_all_inputs()))
def test_shard_stat_is_returns_libs_kernel_order(name):
    """shard_stat repeats kernel_order_stats up to the merged Stat: rounded, it is kernel_order_stats' pair bit for bit, on every shard and whole."""
    a, am, split = _all_inputs()[name]
    for lo, hi in LS.bounds(split) + [(0, a.shape[1])]:
        for asc in (False, True):
            got, want = LS.to_pair(LS.shard_stat(a[:, lo:hi], am[:, lo:hi], asc)), R.kernel_order_stats(a[:, lo:hi], am[:, lo:hi], ascending=asc)
            assert R._same_bits(np.array(got), np.array(want)), (name, lo, hi, asc)


@pytest.mark.parametrize("name", list(_all_inputs()))
def test_emulated_sharded_pair_lies_in_the_candidates_of_the_concatenated_data(name):
    a, am, split = _all_inputs()[name]
    assert sum(split) == a.shape[1]
    pairs = R.candidate_pairs(*R.stats64(a, am))
    for asc in (False, True):
        off = R.pair_offsets(*LS.emulate_returns(a, am, split, asc), pairs)
        print("%s ascending=%d: (dm, dd) = %r" % (name, asc, off))
        assert off is not None, (name, asc)
    if "idle" in name:                                          # the idle shards are idle, and the others are not
        n = [LS.shard_stat(a[:, lo:hi], am[:, lo:hi], True)[0] for lo, hi in LS.bounds(split)]
        assert sorted(x == 0 for x in n) == [False] + [True] * (len(split) - 1)


# which input catches which wrong variant of the returns merge (the others may or may not)
CATCHES_RETURNS = dict(unmerged=("pm100-90+40", "unequal-1+128+64"), mean_of_means=("pm100-90+40", "unequal-1+128+64", "offset-130+idle"),
                       empty_not_skipped=("idle+idle+offset",))


@pytest.mark.parametrize("variant", LS.VARIANTS_RETURNS)
def test_wrong_returns_merges_leave_the_candidates(variant):
    """unmerged (a shard's own statistics) and mean_of_means leave the candidate set wherever the shards differ in mean or size; with an idle shard the
    average of means divides by a shard that has none. empty_not_skipped: Chan's formula happens to pass ONE empty side through unchanged (0 * d), so
    a single idle shard cannot catch it; two idle shards first are 0 / 0, and every later merge is NaN."""
    inputs = _all_inputs()
    for name in CATCHES_RETURNS[variant]:
        a, am, split = inputs[name]
        pairs = R.candidate_pairs(*R.stats64(a, am))
        for asc in (False, True):
            assert R.pair_offsets(*LS.emulate_returns(a, am, split, asc), pairs) is not None
            assert R.pair_offsets(*LS.emulate_returns(a, am, split, asc, variant), pairs) is None, (variant, name, asc)
    if variant == "empty_not_skipped":
        a, am, split = inputs["offset-130+idle"]
        assert LS.emulate_returns(a, am, split, True, variant) == LS.emulate_returns(a, am, split, True)


def test_the_plus_minus_100_shards_have_pairs_of_their_own():
    """What the GPU test relies on: neither shard's own pair normalises to the global result."""
    a, am, split = LS.returns_case("pm100-90+40")
    whole = LS.emulate_returns(a, am, split, True)
    want = R.normalize32(a, *whole)
    for lo, hi in LS.bounds(split):
        alone = R.kernel_order_stats(a[:, lo:hi], am[:, lo:hi], ascending=True)
        assert abs(float(alone[0]) - float(whole[0])) > 50 and not R._same_bits(R.normalize32(a, *alone)[:, lo:hi], want[:, lo:hi])


# ---------------------------------------------------------------------------------------------- (b) PPO loss
VN_CASES = [c for c in LS.LOSS_CASES if LS.FAMILIES[c[0]]["valuenorm"]]


def _emulated(case, variant=None, shard=0):
    inp, c, st, ref = LS.loss_case(case)
    s = LS.global_sums([LS.shard_sums(LS.rows_of(inp, lo, hi)) for lo, hi in LS.bounds(case[2])], variant, shard)
    return inp, c, st, ref, s


@pytest.mark.parametrize("case", LS.LOSS_CASES, ids=LS.loss_case_id)
def test_emulated_global_sums_give_the_restatements_counts_and_state(case):
    inp, c, st, ref, s = _emulated(case)
    assert sum(case[2]) == LS.ROWS == len(inp["returns"]) and s[3] == LS.ROWS
    assert LS.denominators(c, s) == (ref["denom_policy"], ref["denom_value"])
    if case[3] == "one_active":
        lo, hi = LS.bounds(case[2])[1]
        assert inp["active_masks"][lo:hi].sum() == 0 and inp["active_masks"].sum() > 0
    if case[3] == "pm100":
        for i, (lo, hi) in enumerate(LS.bounds(case[2])):
            assert abs(float(inp["returns"][lo:hi].mean()) - (100.0 if i == 0 else -100.0)) < 5
    if c.use_valuenorm:
        got = LS.valuenorm_update32(st, s)
        for k, v in ref["state"].items():
            assert abs(float(got[k]) - float(v.reshape(-1)[0])) <= LS.state_tolerance(inp, k), (k, float(got[k]), float(v.reshape(-1)[0]))
        assert not P.undecided(inp, c, st).any()


def test_loss_cases_stay_where_the_bound_was_derived():
    """C_DEV = 4 * C_REF, C_REF being the error of the reference's own float32 arithmetic: every sharded case must leave that arithmetic inside C_REF."""
    worst = {}
    for case in LS.LOSS_CASES:
        inp, c, st, ref = LS.loss_case(case)
        worst[LS.loss_case_id(case)] = P.reference_error(P.restate(inp, c, torch.float32, st), ref)
    print(", ".join("%s %.1f" % kv for kv in worst.items()))
    assert max(worst.values()) <= P.C_REF, worst


# which case catches which wrong variant: (case, the shard whose own numbers are used, what goes wrong)
PM100 = ("on_vn", 25, (257, 773), "pm100")
ONE_ACTIVE = ("on_vn", 5, (257, 773), "one_active")
PLAIN_OFF = ("off_vn", 5, (257, 773), None)


def test_wrong_loss_sums_are_told_apart():
    """unmerged: a shard's own sums move the ValueNorm state outside the tolerance where the shards' returns differ (pm100), and give a zero
    denominator on the shard that holds no active row (one_active). local_rows: with the means over all rows (flags off) the denominators are the
    shard's row count, not the minibatch's, and the batch means fed to ValueNorm.update are scaled by rows / shard rows."""
    assert PM100 in LS.LOSS_CASES and ONE_ACTIVE in LS.LOSS_CASES and PLAIN_OFF in LS.LOSS_CASES
    for shard in (0, 1):
        inp, c, st, ref, s = _emulated(PM100, "unmerged", shard)
        bad = LS.valuenorm_update32(st, s)
        assert abs(float(bad["running_mean"]) - float(ref["state"]["running_mean"].reshape(-1)[0])) > 5 * LS.state_tolerance(inp, "running_mean")
    inp, c, st, ref, s = _emulated(ONE_ACTIVE, "unmerged", 1)
    assert LS.denominators(c, s) == (0.0, 0.0) and ref["denom_policy"] > 0
    for shard in (0, 1):
        inp, c, st, ref, s = _emulated(PLAIN_OFF, "local_rows", shard)
        assert LS.denominators(c, s) == (float(PLAIN_OFF[2][shard]),) * 2 != (ref["denom_policy"], ref["denom_value"])
        bad = LS.valuenorm_update32(st, s)
        off = abs(float(bad["running_mean_sq"]) - float(ref["state"]["running_mean_sq"].reshape(-1)[0])) / LS.state_tolerance(inp, "running_mean_sq")
        assert off > (5 if shard == 0 else 1), (shard, off)         # the small shard's batch means are 4x too large, the large shard's by a third
    # the ratio mean: a shard's sum of ratios over its own row count, added over the shards, is about `world` times too large
    parts = [float(ref["imp_weights"][lo:hi].sum()) for lo, hi in LS.bounds(PLAIN_OFF[2])]
    good, local = sum(p / LS.ROWS for p in parts), sum(p / n for p, n in zip(parts, PLAIN_OFF[2]))
    bound = P.scalar_bounds(ref, P.C_DEV)["ratio_mean"]
    assert abs(good - float(ref["ratio_mean"])) <= bound and abs(local - float(ref["ratio_mean"])) > 100 * bound


# ---------------------------------------------------------------------------------------------- (c)
def _exchange_worker(rank, world, path, q):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method="file://" + path, rank=rank, world_size=world)
    try:
        from gmpe.learner_shards import ProcessGroupExchange, gather
        x = ProcessGroupExchange()
        out = []
        for k in (3, 4):
            local = torch.arange(k, dtype=torch.float64) + 10.0 * (rank + 1)
            out.append(gather(x, local, "test").numpy().copy())
        sub = ProcessGroupExchange(dist.new_group([0, 1]))
        q.put((rank, x.world, x.rank, sub.world, sub.rank, out))
    finally:
        dist.destroy_process_group()


def test_process_group_exchange_gathers_in_rank_order_over_gloo():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with tempfile.TemporaryDirectory() as t:
        ps = [ctx.Process(target=_exchange_worker, args=(r, 2, os.path.join(t, "store"), q)) for r in range(2)]
        for p in ps:
            p.start()
        got = sorted(q.get(timeout=120) for _ in ps)
        for p in ps:
            p.join(timeout=60)
            assert p.exitcode == 0
    for rank, (r, world, xr, sw, sr, out) in enumerate(got):
        assert (r, world, xr, sw, sr) == (rank, 2, rank, 2, rank)
        for k, a in zip((3, 4), out):
            assert a.dtype == np.float64 and a.shape == (2, k)
            np.testing.assert_array_equal(a, np.arange(k)[None, :] + np.array([[10.0], [20.0]]))       # row r is rank r's, on both ranks


def test_process_group_exchange_needs_a_process_group():
    with pytest.raises(RuntimeError, match="initialised"):
        gmpe.learner_shards.ProcessGroupExchange()
    assert gmpe.ProcessGroupExchange is gmpe.learner_shards.ProcessGroupExchange


# ---------------------------------------------------------------------------------------------- (d)
class _Stack(object):
    """An exchange that needs no process group: this process is every rank."""

    def __init__(self, world=2, rank=0, rows=None):
        self.world, self.rank, self.rows = world, rank, rows

    def exchange(self, local):
        return torch.stack([local] * (self.world if self.rows is None else self.rows))


def _returns_handle(done=False):
    h = gmpe.engine.ReturnsShard(_lib.GmpeReturnsShardPlan(), torch.device("cpu"), (), torch.zeros(3, 2, 1), torch.zeros(3, dtype=torch.float64))
    h.done = done
    return h


def _loss_handle(done=False):
    call = types.SimpleNamespace(dev=torch.device("cpu"))
    h = gmpe.ppo_loss.PPOLossShard(call, _lib.GmpePpoLossShardPlan(), torch.zeros(4, dtype=torch.float64))
    h.done = done
    return h


BAD_STATS = [(lambda k: torch.zeros(k, dtype=torch.float64), "shape"), (lambda k: torch.zeros(2, k + 1, dtype=torch.float64), "shape"),
             (lambda k: torch.zeros(2, k), "float64"), (lambda k: torch.zeros(0, k, dtype=torch.float64), "outside 1"),
             (lambda k: torch.zeros(4097, k, dtype=torch.float64), "outside 1"), (lambda k: torch.zeros(2, k, dtype=torch.float64, device="meta"), "must be on"),
             (lambda k: torch.zeros(k, 2, dtype=torch.float64).t(), "contiguous"), (lambda k: np.zeros((2, k)), "shape")]


@pytest.mark.parametrize("make,match", BAD_STATS, ids=[m + str(i) for i, (_, m) in enumerate(BAD_STATS)])
def test_finish_refuses_bad_all_stats_before_any_launch(make, match):
    for finish, handle, k in ((gmpe.compute_returns_finish, _returns_handle, 3), (gmpe.ppo_losses_finish, _loss_handle, 4)):
        h = handle()
        with pytest.raises(ValueError, match=match):
            finish(h, make(k))
        assert not h.done
        with pytest.raises(ValueError, match="no CPU fallback"):        # everything else in order: only the device is missing
            finish(h, torch.zeros(2, k, dtype=torch.float64))
        assert not h.done


def test_finish_refuses_a_second_call_and_a_foreign_handle():
    for finish, handle, k in ((gmpe.compute_returns_finish, _returns_handle, 3), (gmpe.ppo_losses_finish, _loss_handle, 4)):
        with pytest.raises(RuntimeError, match="already called"):
            finish(handle(done=True), torch.zeros(2, k, dtype=torch.float64))
        with pytest.raises(TypeError, match="must come from"):
            finish(object(), torch.zeros(2, k, dtype=torch.float64))
    with pytest.raises(ValueError, match="reduce must be"):
        gmpe.ppo_losses_finish(_loss_handle(), torch.zeros(2, 4, dtype=torch.float64), reduce="avg")


def _returns_kw(T=3, L=4):
    z = lambda *s: torch.zeros(*s)
    return dict(rewards=z(T, L, 1), masks=z(T + 1, L, 1), value_preds=z(T + 1, L, 1), returns=z(T + 1, L, 1), next_value=z(L, 1), advantages=z(T, L, 1),
                active_masks=z(T + 1, L, 1), normalized=z(T, L, 1))


def test_begin_and_the_one_call_forms_refuse_bad_arguments_before_any_launch():
    from test_ppo_loss_host import _sample
    kw = _returns_kw()
    with pytest.raises(ValueError, match="normalized .* required"):
        gmpe.compute_returns_begin(**dict(kw, normalized=None))
    with pytest.raises(ValueError, match="normalized .* required"):
        gmpe.engine.compute_returns(shards=_Stack(), **dict(kw, normalized=None))
    with pytest.raises(ValueError, match="active_masks"):
        gmpe.compute_returns_begin(**dict(kw, active_masks=None))
    with pytest.raises(ValueError, match="rewards must be"):
        gmpe.compute_returns_begin(**dict(kw, rewards=torch.zeros(2, 4, 1)))
    with pytest.raises(ValueError, match="no CPU fallback"):
        gmpe.compute_returns_begin(**kw)
    args = types.SimpleNamespace(use_valuenorm=False)
    lg, vl = torch.zeros(6, 5), torch.zeros(6, 1)
    with pytest.raises(ValueError, match="returns must have shape"):
        gmpe.ppo_losses_begin(lg, vl, _sample(returns=torch.zeros(5, 1)), args)
    with pytest.raises(ValueError, match="value_normalizer"):
        gmpe.ppo_losses_begin(lg, vl, _sample(), types.SimpleNamespace(use_valuenorm=True))
    with pytest.raises(ValueError, match="no CPU fallback"):
        gmpe.ppo_losses_begin(lg, vl, _sample(), args)
    for bad, exc in ((object(), TypeError), (_Stack(world=0), ValueError), (_Stack(world=4097), ValueError), (_Stack(world=2, rank=2), ValueError)):
        with pytest.raises(exc, match="shards"):
            gmpe.engine.compute_returns(shards=bad, **kw)
        with pytest.raises(exc, match="shards"):
            gmpe.ppo_losses(lg, vl, _sample(), args, shards=bad)
    with pytest.raises(ValueError, match="reduce must be"):
        gmpe.ppo_losses(lg, vl, _sample(), args, shards=_Stack(), reduce="avg")
    with pytest.raises(ValueError, match="returned 3 rows"):
        gmpe.learner_shards.gather(_Stack(world=2, rows=3), torch.zeros(4, dtype=torch.float64), "test")
    with pytest.raises(NotImplementedError, match="PopArt variant has no sharded form"):
        gmpe.ppo_losses_popart(lg, torch.zeros(6, 8), _sample(), types.SimpleNamespace(use_popart=True), None, shards=_Stack())


def test_buffer_methods_take_shards():
    import inspect
    from gmpe.rollout import DeviceRolloutBuffer
    for f in (DeviceRolloutBuffer.compute_returns, DeviceRolloutBuffer.normalized_advantages, gmpe.engine.compute_returns, gmpe.ppo_losses):
        assert inspect.signature(f).parameters["shards"].default is None
    assert inspect.signature(gmpe.ppo_losses).parameters["reduce"].default == "sum"
