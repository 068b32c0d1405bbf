"""The sharded gmpe.clip_and_step (include/gmpe.h gmpe_optim_step_shard) and shards= of gmpe.policy.ppo_update / train on the device. The shards of a
data-parallel learner are emulated in one process, as in tests/test_gpu_learner_shards.py: begin on every replica, torch.stack of the `.local`s, finish on
every replica — or, for the one-call forms, replicas on threads joined by tests/optim_shards_lib.py's lockstep exchange.

The combination rule is restated in numpy (optim_shards_lib.fold: a float64 left fold over the ranks, rounded once); what follows the sum is the existing
clip_and_step, so the step is compared bit for bit with that call on a fresh replica handed the restated sum, and needs no tolerance. Only the comparison
of a sharded update with the unsharded one over the same rows has one: the project's accuracy rule against float64 torch."""
import copy
import ctypes as C
import types

import numpy as np
import pytest
import torch

import gmpe
import head_lib as HL
import optim_lib as OL
import optim_shards_lib as SL
from gmpe import _lib, policy
from test_gpu_optim import bits, same
from test_gpu_policy import DEV, L, NB, sample_of
from test_gpu_ppo_update import A, EPS, LR, N, _train_args, _train_nets, equal_dicts, everything, nets, update_args

pytestmark = pytest.mark.gpu
STATE = ("exp_avg", "exp_avg_sq")


def replica(params, wd=1e-2):
    ps = OL.torch_params(params, device=DEV)
    return ps, torch.optim.Adam(ps, lr=OL.LR, eps=OL.EPS, weight_decay=wd)


def sharded(reps, per_rank, max_norm, **kw):
    """one sharded call over the replicas [(ps, opt)] with the ranks' gradients [rank][tensor] -> (what finish returned per replica, the handles, all)"""
    for (ps, _), g in zip(reps, per_rank):
        OL.set_grads(ps, g)
    hs = [gmpe.clip_and_step_begin(opt, max_norm, **kw) for _, opt in reps]
    all_ = torch.stack([h.local for h in hs])
    return [gmpe.clip_and_step_finish(h, all_) for h in hs], hs, all_


def same_replica(a, b, what, step=True):
    """two replicas (ps, opt): parameters, gradients, Adam state and step counts bit for bit"""
    (pa, oa), (pb, ob) = a, b
    for i, (p, q) in enumerate(zip(pa, pb)):
        assert same(p, q) and same(p.grad, q.grad), (what, i)
        assert bool(oa.state[p]) == bool(ob.state[q]) == bool(step), (what, i)
        if step:
            assert float(oa.state[p]["step"]) == float(ob.state[q]["step"]) and oa.state[p]["step"].device.type == "cpu", (what, i)
            for k in STATE:
                assert same(oa.state[p][k], ob.state[q][k]), (what, i, k)


# ---------------------------------------------------------------------------------------------- 1, 3, 5
@pytest.mark.parametrize("mode", ["bites", "loose", "none", "clip-only"])
@pytest.mark.parametrize("world", SL.WORLDS)
def test_the_sum_is_the_restated_one_and_the_step_is_the_existing_call_on_it(world, mode):
    max_norm = {"bites": 1e-3, "loose": 1e9, "none": None, "clip-only": 1e-3}[mode]
    step = mode != "clip-only"
    for shapes, seed in ((SL.SHAPES, 1), (SL.MANY, 2)):
        params = OL.parameters(shapes, seed)
        reps, plain = [replica(params) for _ in range(world)], replica(params)
        for k in range(2):
            per_rank = SL.rank_gradients(shapes, world, k, seed)
            want = SL.summed(per_rank)
            norms, hs, all_ = sharded(reps, per_rank, max_norm, step=step)
            OL.set_grads(plain[0], want)
            pnorm = gmpe.clip_and_step(plain[1], max_norm, step=step)
            torch.cuda.synchronize()
            # LOCAL packed this rank's gradients back to back, in table order
            for r in range(world):
                assert np.array_equal(bits(all_[r]), np.concatenate([bits(g) for g in per_rank[r]])), (k, r)
                assert hs[r].local.dtype == torch.float32 and tuple(hs[r].local.shape) == (sum(int(np.prod(s)) for s in shapes),)
            for r in range(world):
                assert norms[r].dtype == torch.float32 and norms[r].dim() == 0 and same(norms[r], pnorm), (k, r)
                same_replica(reps[r], plain, (world, mode, k, r), step)
                if mode in ("loose", "none"):               # nothing is scaled (a factor of 1 keeps the bits): p.grad is the restated sum
                    assert all(same(p.grad, g) for p, g in zip(reps[r][0], want)), (k, r)
            if mode == "bites":
                assert float(pnorm) > max_norm and not same(plain[0][1].grad, want[1])
            if world > 1:
                assert not same(want[1], per_rank[0][1])


def test_world_1_is_the_plain_call_bit_for_bit():
    params = OL.parameters(SL.SHAPES, 3)
    grads = OL.gradients(SL.SHAPES, 0, 3)
    one, plain = replica(params), replica(params)
    OL.set_grads(one[0], grads)
    OL.set_grads(plain[0], grads)
    h = gmpe.clip_and_step_begin(one[1], 1e-3)
    assert not any(one[1].state[p] for p in one[0]) and all(same(p.grad, g) for p, g in zip(one[0], grads))      # begin creates nothing and changes nothing
    norm = gmpe.clip_and_step_finish(h, h.local.unsqueeze(0))
    pnorm = gmpe.clip_and_step(plain[1], 1e-3)
    assert same(norm, pnorm)
    same_replica(one, plain, "world 1")
    with pytest.raises(RuntimeError, match="already called"):
        gmpe.clip_and_step_finish(h, h.local.unsqueeze(0))
    assert all(float(one[1].state[p]["step"]) == 1 for p in one[0])


# ---------------------------------------------------------------------------------------------- 2
def test_rank_order_double_precision_and_every_rank_show_in_the_sum():
    cols = (SL.BIG, SL.SWAPPED, SL.CANCEL, SL.KEEPS)
    per_rank = [[np.array([c[r] for c in cols], np.float32)] for r in range(3)]
    want = SL.summed(per_rank)[0]
    assert want.tolist() == [1.0, 0.0, 0.25, 3.0]
    reps = [replica([np.zeros(4, np.float32)]) for _ in range(3)]
    norms, _, _ = sharded(reps, per_rank, None, step=False)
    for (ps, _), norm in zip(reps, norms):
        assert same(ps[0].grad, want)
        assert float(norm) == float(np.float32(np.sqrt(1.0 + 0.0625 + 9.0)))
    # a negative zero in every rank stays one: the fold starts at rank 0's value
    reps = [replica([np.zeros(2, np.float32)]) for _ in range(2)]
    sharded(reps, [[np.array([-0.0, -0.0], np.float32)], [np.array([-0.0, 0.0], np.float32)]], None, step=False)
    assert bits(reps[0][0][0].grad).tolist() == [0x80000000, 0]


# ---------------------------------------------------------------------------------------------- 4
def test_a_plain_call_after_a_sharded_one_in_the_same_workspace_is_the_fresh_plain_call():
    params = OL.parameters(SL.SHAPES, 4)
    ws = torch.full((1 << 12,), 0xA5, dtype=torch.uint8, device=DEV)
    reps = [replica(params) for _ in range(2)]
    sharded(reps, SL.rank_gradients(SL.SHAPES, 2, 0, 4), 1e-3, workspace=ws)
    grads = OL.gradients(SL.SHAPES, 1, 4)
    used, fresh = replica(params), replica(params)
    OL.set_grads(used[0], grads)
    OL.set_grads(fresh[0], grads)
    a, b = gmpe.clip_and_step(used[1], 1e-3, workspace=ws), gmpe.clip_and_step(fresh[1], 1e-3)
    assert same(a, b)
    same_replica(used, fresh, "after a sharded call")


# ---------------------------------------------------------------------------------------------- 6
def _sets(params, grads):
    """a: no gradient; b: in both; c: in `parameters` only; d: in the optimiser only; e: no elements"""
    a, b, c, d, e = ps = OL.torch_params(params, device=DEV)
    OL.set_grads(ps, [None] + list(grads[1:]))
    return ps, torch.optim.Adam([a, b, d, e], lr=OL.LR, eps=OL.EPS), [a, b, c, e]


def test_the_clipped_set_and_the_stepped_set_may_differ():
    shapes = ((7,), (40, 30), (OL.CHUNK + 5,), (33,), (0,))
    params = OL.parameters(shapes, 5)
    per_rank = SL.rank_gradients(shapes, 3, 0, 5)
    want = SL.summed(per_rank)
    reps = [_sets(params, g) for g in per_rank]
    hs = [gmpe.clip_and_step_begin(opt, 2.0, parameters=normed) for _, opt, normed in reps]
    assert all(tuple(h.local.shape) == (40 * 30 + OL.CHUNK + 5 + 33,) for h in hs)          # b, d, then c: the optimiser's own first
    all_ = torch.stack([h.local for h in hs])
    norms = [gmpe.clip_and_step_finish(h, all_) for h in hs]
    ps, opt, normed = _sets(params, want)
    pnorm = gmpe.clip_and_step(opt, 2.0, parameters=normed)
    assert float(pnorm) > 2.0
    for (qs, qopt, _), norm in zip(reps, norms):
        assert same(norm, pnorm)
        for i, (p, q) in enumerate(zip(ps, qs)):
            assert same(p, q) and (p.grad is None) == (q.grad is None) and (p.grad is None or same(p.grad, q.grad)), i
            assert (p in opt.state and bool(opt.state[p])) == (q in qopt.state and bool(qopt.state[q])), i
            if p in opt.state and opt.state[p]:
                assert all(same(opt.state[p][k], qopt.state[q][k]) for k in STATE) and float(qopt.state[q]["step"]) == 1, i
        a, b, c, d, e = qs
        assert a not in qopt.state and c not in qopt.state and same(c, params[2]) and not same(c.grad, want[2])      # c: scaled only
        assert same(d.grad, want[3]) and not same(d, params[3])                                                  # d: stepped on the sum, unscaled
    # nothing has a gradient on any rank: nothing to exchange, the norm of nothing, also through the one-call form
    for qs, _, _ in reps:
        for p in qs:
            p.grad = None
    h = gmpe.clip_and_step_begin(reps[0][1], 2.0, parameters=reps[0][2], step=False)
    assert h.local.numel() == 0 and float(gmpe.clip_and_step_finish(h, h.local.new_empty((3, 0)))) == 0.0
    x = SL.Lockstep(1)
    zero = gmpe.clip_and_step(reps[0][1], 2.0, parameters=reps[0][2], shards=x.rank(0))
    assert float(zero) == 0.0 and zero.dtype == torch.float32 and zero.device.type == "cuda" and x.calls == [0]


# ---------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("k", [1, 6, 16])
def test_extra_comes_back_as_the_restated_sums(k):
    world = 3
    params = OL.parameters(SL.SHAPES, 6)
    per_rank = SL.rank_gradients(SL.SHAPES, world, 0, 6)
    rng = np.random.RandomState(60 + k)
    extras = [(rng.randn(k) * 10.0 ** rng.randint(-3, 4, k)).astype(np.float32) for _ in range(world)]
    reps, plain = [replica(params) for _ in range(world)], replica(params)
    for (ps, _), g in zip(reps, per_rank):
        OL.set_grads(ps, g)
    given = [torch.from_numpy(e).to(DEV) for e in extras]
    hs = [gmpe.clip_and_step_begin(opt, 1e-3, extra=x) for (_, opt), x in zip(reps, given)]
    n = sum(SL.SIZES)
    all_ = torch.stack([h.local for h in hs])
    assert tuple(all_.shape) == (world, n + k) and all(np.array_equal(bits(all_[r, n:]), bits(extras[r])) for r in range(world))
    outs = [gmpe.clip_and_step_finish(h, all_) for h in hs]
    OL.set_grads(plain[0], SL.summed(per_rank))
    pnorm = gmpe.clip_and_step(plain[1], 1e-3)
    for r, (norm, total) in enumerate(outs):
        assert same(norm, pnorm) and same(total, SL.fold(extras)) and tuple(total.shape) == (k,) and total.dtype == torch.float32
        assert same(given[r], extras[r])                    # the caller's tensor is left alone
        same_replica(reps[r], plain, ("extra", r))          # and the step does not see it
    # extra alone, where no tensor has a gradient: the exchange still happens, the norm is that of nothing
    for ps, _ in reps:
        for p in ps:
            p.grad = None
    hs = [gmpe.clip_and_step_begin(opt, None, step=False, extra=x) for (_, opt), x in zip(reps, given)]
    all_ = torch.stack([h.local for h in hs])
    assert tuple(all_.shape) == (world, k)
    for h in hs:
        norm, total = gmpe.clip_and_step_finish(h, all_)
        assert float(norm) == 0.0 and same(total, SL.fold(extras))


# ---------------------------------------------------------------------------------------------- 8
def test_a_nan_in_one_ranks_gradient_reaches_every_replica_alike():
    params = OL.parameters(SL.SHAPES, 7)
    per_rank = SL.rank_gradients(SL.SHAPES, 3, 0, 7)
    per_rank[1][3][2000] = np.nan
    reps = [replica(params) for _ in range(3)]
    norms, _, _ = sharded(reps, per_rank, 1e-3)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(n)) for n in norms) and all(same(n, norms[0]) for n in norms)
    for r in (1, 2):
        same_replica(reps[r], reps[0], ("nan", r))
    assert bool(torch.isnan(reps[0][0][3].grad).all()) and bool(torch.isnan(reps[2][0][0]).all())       # coef is NaN: every clipped gradient and every step


# ---------------------------------------------------------------------------------------------- 9
def test_the_c_entry_with_unaligned_starts_packs_straight_into_the_rows_of_all():
    lib = _lib.load()
    world, sizes = 3, (5, OL.CHUNK - 1, OL.CHUNK + 1, 77)
    shapes = tuple((s,) for s in sizes)
    n = sum(sizes)
    params, per_rank = OL.parameters(shapes, 9), SL.rank_gradients(shapes, world, 0, 9)
    plain = replica(params)
    OL.set_grads(plain[0], SL.summed(per_rank))
    MN = 1e-3
    pnorm = gmpe.clip_and_step(plain[1], MN)
    GUARD = 7.25
    offs = {"param": 3, "grad": 5, "exp_avg": 1, "exp_avg_sq": 7}
    bufs = {k: [torch.full((s + 16,), GUARD, device=DEV) for s in sizes] for k in offs}
    view = lambda k, i: bufs[k][i][offs[k]:offs[k] + sizes[i]]
    all_buf = torch.full((world * n + 16,), GUARD, device=DEV)           # the rows start 1, 1 + n, 1 + 2n floats in: 4-byte aligned and no more
    ALL0 = 1
    for i in range(len(sizes)):
        view("param", i).copy_(torch.from_numpy(params[i]))
        view("exp_avg", i).zero_()
        view("exp_avg_sq", i).zero_()
    ts = (_lib.GmpeOptimTensor * len(sizes))()
    for i in range(len(sizes)):
        ts[i].param, ts[i].grad, ts[i].exp_avg, ts[i].exp_avg_sq = (view(k, i).data_ptr() for k in ("param", "grad", "exp_avg", "exp_avg_sq"))
        ts[i].numel, ts[i].flags, ts[i].hyper = sizes[i], _lib.OPT_T_IN_NORM | _lib.OPT_T_STEP, 0
        assert ts[i].grad % 16 != 0
    hs = (_lib.GmpeOptimHyper * 1)()
    hs[0].lr, hs[0].beta1, hs[0].beta2, hs[0].eps, hs[0].weight_decay, hs[0].t = OL.LR, 0.9, 0.999, OL.EPS, 1e-2, 1
    sp = _lib.GmpeOptimShardPlan()
    b = sp.base
    b.n_tensors, b.n_hypers, b.tensors, b.hypers, b.flags, b.max_norm = len(sizes), 1, ts, hs, _lib.OPT_CLIP | _lib.OPT_STEP, MN
    need, ne = C.c_size_t(), C.c_int64()
    assert lib.gmpe_optim_workspace_bytes(C.byref(b), C.byref(need)) == 0 and lib.gmpe_optim_shard_elems(C.byref(b), C.byref(ne)) == 0 and ne.value == n
    out, f32 = torch.zeros(2, dtype=torch.float64, device=DEV), torch.zeros(1, device=DEV)
    ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    b.out, b.grad_norm_f32, b.workspace, b.workspace_bytes = out.data_ptr(), f32.data_ptr(), ws.data_ptr(), need.value
    sp.world, sp.local_elems = world, n
    stream = torch.cuda.current_stream(DEV).cuda_stream
    for r in range(world):                                               # LOCAL of rank r writes row r of `all` itself
        for i in range(len(sizes)):
            view("grad", i).copy_(torch.from_numpy(per_rank[r][i]))
        sp.phase, sp.local = _lib.SHARD_LOCAL, all_buf.data_ptr() + 4 * (ALL0 + r * n)
        assert sp.local % 8 != 0 or r > 0
        assert lib.gmpe_optim_step_shard(0, C.byref(sp), C.c_void_p(stream)) == 0, lib.gmpe_last_error()
    sp.phase, sp.all = _lib.SHARD_APPLY, all_buf.data_ptr() + 4 * ALL0
    assert lib.gmpe_optim_step_shard(0, C.byref(sp), C.c_void_p(stream)) == 0, lib.gmpe_last_error()
    torch.cuda.synchronize()
    whole = all_buf.cpu().numpy()
    assert (whole[:ALL0] == GUARD).all() and (whole[ALL0 + world * n:] == GUARD).all()
    for r in range(world):
        assert np.array_equal(bits(whole[ALL0 + r * n:ALL0 + (r + 1) * n]), np.concatenate([bits(g) for g in per_rank[r]])), r
    assert same(f32[0], pnorm) and float(out[0]) > MN
    for i, s in enumerate(sizes):
        want = {"param": plain[0][i], "grad": plain[0][i].grad, "exp_avg": plain[1].state[plain[0][i]]["exp_avg"],
                "exp_avg_sq": plain[1].state[plain[0][i]]["exp_avg_sq"]}
        for k in offs:
            w = bufs[k][i].cpu().numpy()
            assert (w[:offs[k]] == GUARD).all() and (w[offs[k] + s:] == GUARD).all(), (k, i)
            assert same(w[offs[k]:offs[k] + s], want[k]), (k, i)


# ---------------------------------------------------------------------------------------------- 10 - 13: ppo_update and train
CUT = 2                                 # the sequences of the sample go 2 : 3 to the two replicas: 12 and 18 rows


def shard_of(s, lo, hi):
    """sequences lo .. hi of the time-major 16-tuple: [L * NB, ...] fields by their row's sequence, the two RNN states [NB, 1, 64] by row"""
    cut = lambda t: t.reshape((L, NB) + tuple(t.shape[1:]))[:, lo:hi].reshape((L * (hi - lo),) + tuple(t.shape[1:])).contiguous()
    return tuple(t[lo:hi].contiguous() if i in (6, 7) else cut(t) for i, t in enumerate(s))


def shards_of(s):
    return [shard_of(s, 0, CUT), shard_of(s, CUT, NB)]


def by_hand(reps, samples, args):
    """ppo_update(shards=...) on every replica, written out: minibatch_losses' parts around ppo_losses_begin / _finish, then the two
    clip_and_step_begin / _finish pairs, the scalars riding on the critic's"""
    F = torch.nn.functional
    hs = []
    for (actor, critic, _, _), s in zip(reps, samples):
        nbd = gmpe.gnn_base(s[2], s[3], s[4], actor.gnn_base)
        f, _ = gmpe.rnn_layer(gmpe.mlp_base((s[1], nbd), actor.base), s[6], s[11], actor.rnn)
        logits = gmpe.action_logits(f, actor.act)
        nbd_c = gmpe.gnn_base(s[2], s[3], s[5], critic.gnn_base)
        fc, _ = gmpe.rnn_layer(gmpe.mlp_base((s[0], nbd_c), critic.base), s[7], s[11], critic.rnn)
        hs.append(gmpe.ppo_losses_begin(logits, F.linear(fc, critic.v_out.weight, critic.v_out.bias), s, args))
    stats = torch.stack([h.local for h in hs])
    res = [gmpe.ppo_losses_finish(h, stats) for h in hs]
    ha = []
    for (actor, _, aopt, _), r in zip(reps, res):
        aopt.zero_grad()
        r.actor_loss.backward()
        ha.append(gmpe.clip_and_step_begin(aopt, args.max_grad_norm, parameters=actor.parameters()))
    all_a = torch.stack([h.local for h in ha])
    an = [gmpe.clip_and_step_finish(h, all_a) for h in ha]
    hc = []
    for (_, critic, _, copt), r in zip(reps, res):
        copt.zero_grad()
        (r.value_loss * args.value_loss_coef).backward()
        w = r.imp_weights.detach()
        extra = torch.stack((r.value_loss.detach(), r.policy_loss.detach(), r.dist_entropy.detach(), r.ratio_mean.detach(), w.sum(),
                             w.new_full((), float(w.numel()))))
        hc.append(gmpe.clip_and_step_begin(copt, args.max_grad_norm, parameters=critic.parameters(), extra=extra))
    all_c = torch.stack([h.local for h in hc])
    out = []
    for h, r, a in zip(hc, res, an):
        cn, t = gmpe.clip_and_step_finish(h, all_c)
        out.append(policy.PPOUpdate(t[0], cn, t[1], t[2], a, t[3], r.imp_weights.detach()))
    return out


def test_ppo_update_with_shards_is_the_sequence_written_out_and_the_replicas_stay_equal():
    s, args = sample_of(), update_args()
    samples = shards_of(s)
    assert [int(x[1].shape[0]) for x in samples] == [12, 18]
    hand = [nets() for _ in range(2)]
    us_hand = by_hand(hand, samples, args)
    call = [nets() for _ in range(2)]
    x = SL.Lockstep(2)
    us_call = x.run(lambda r, sh: policy.ppo_update(*call[r], samples[r], args, shards=sh))
    torch.cuda.synchronize()
    assert x.calls == [3, 3]                                # the loss statistics, the actor's gradients, the critic's with the scalars
    states = [everything(*rep) for rep in hand + call]
    for other in states[1:]:
        equal_dicts(states[0], other)                       # (b) is (a), and both replicas are each other, bit for bit
    start = everything(*nets())
    assert sum(not same(start[k], states[0][k]) for k in start if k.startswith(("actor.", "critic."))) > 40
    for u in us_hand + us_call:
        assert isinstance(u, policy.PPOUpdate)
        for k in u._fields[:6]:
            t = getattr(u, k)
            assert t.dim() == 0 and t.dtype == torch.float32 and t.device.type == "cuda" and not t.requires_grad and bool(torch.isfinite(t)), k
            assert same(t, getattr(us_hand[0], k)), k       # the whole minibatch's scalars, the same on both replicas and in both forms
        assert float(u.actor_grad_norm) > args.max_grad_norm and float(u.critic_grad_norm) > args.max_grad_norm
    for r in range(2):                                      # imp_weights stays the replica's own rows
        assert tuple(us_call[r].imp_weights.shape) == (samples[r][1].shape[0], 1) and same(us_call[r].imp_weights, us_hand[r].imp_weights)
    # p.grad holds the global gradient afterwards, clipped, the same on both replicas
    for p, q in zip(call[0][0].parameters(), call[1][0].parameters()):
        assert same(p.grad, q.grad)
    # the scalars are those of the whole minibatch: the unsharded update reports them up to rounding
    whole = policy.ppo_update(*nets(), s, args)
    for k in whole._fields[:6]:
        a, b = float(getattr(us_call[0], k)), float(getattr(whole, k))
        assert abs(a - b) <= 1e-4 * max(1.0, abs(b)), (k, a, b)
    # update_actor=False: the actor's call exchanges nothing (no tensor has a gradient, on either replica), the critic's still carries the scalars
    again = [nets() for _ in range(2)]
    x = SL.Lockstep(2)
    us = x.run(lambda r, sh: policy.ppo_update(*again[r], samples[r], args, update_actor=False, shards=sh))
    assert x.calls == [2, 2] and all(float(u.actor_grad_norm) == 0.0 for u in us) and len(again[0][2].state) == 0
    for k in start:
        if k.startswith(("actor.", "aopt.")):
            assert same(start[k], everything(*again[1])[k]), k


FMIN32 = float(np.finfo(np.float32).min)


def loss64(logits, values, s, args):
    """the loss arithmetic of GR_MAPPO.ppo_update (graph_mappo.py:176-207, cal_value_loss :89-117) in torch, in the dtype of logits, for loss_args' flags:
    active masks in both means, the clipped value loss, the reference's one-sided Huber, no value normaliser -> (actor_loss, value_loss)"""
    act, vp, ret, am, old, adv, avail = s[8].long().view(-1), s[9], s[10], s[12], s[13], s[14], s[15]
    dist = torch.distributions.Categorical(logits=torch.where(avail == 0, torch.full_like(logits, FMIN32), logits))
    logp, ent = dist.log_prob(act).unsqueeze(-1), dist.entropy()
    dist_entropy = (ent * am.squeeze(-1)).sum() / am.sum()
    ratio = torch.exp(logp - old)
    surr = torch.min(ratio * adv, torch.clamp(ratio, 1.0 - args.clip_param, 1.0 + args.clip_param) * adv)
    policy_loss = (-surr * am).sum() / am.sum()
    vpc = vp + (values - vp).clamp(-args.clip_param, args.clip_param)
    d = args.huber_delta
    huber = lambda e: (abs(e) <= d).to(e.dtype) * e ** 2 / 2 + (e > d).to(e.dtype) * d * (abs(e) - d / 2)
    value_loss = (torch.max(huber(ret - values), huber(ret - vpc)) * am).sum() / am.sum()
    return policy_loss - dist_entropy * args.entropy_coef, value_loss


def update64(s, args):
    """one ppo_update over the whole sample in float64 torch on the CPU -> everything()'s dict"""
    actor, critic, _, _ = nets()
    actor, critic = copy.deepcopy(actor).cpu().double(), copy.deepcopy(critic).cpu().double()
    s = tuple(t.cpu().double() if t.is_floating_point() else t.cpu() for t in s)
    adam = lambda net: torch.optim.Adam(list(net.parameters()), lr=LR, eps=EPS, weight_decay=0)
    aopt, copt = adam(actor), adam(critic)
    fa, _ = actor.torch_forward(s[1], s[2], s[3], s[4], s[6], s[11], L)
    fc, _ = critic.torch_forward(s[0], s[2], s[3], s[5], s[7], s[11], L)
    actor_loss, value_loss = loss64(actor.head_linear()(fa), critic.head_linear()(fc), s, args)
    actor_loss.backward()
    torch.nn.utils.clip_grad_norm_(actor.parameters(), args.max_grad_norm)
    aopt.step()
    (value_loss * args.value_loss_coef).backward()
    torch.nn.utils.clip_grad_norm_(critic.parameters(), args.max_grad_norm)
    copt.step()
    return everything(actor, critic, aopt, copt)


def test_the_sharded_update_meets_the_accuracy_rule_like_the_unsharded_one():
    """err = max|a - a64| / max(1, max|a64|) per parameter and state array after one update, a64 from float64 torch over the whole minibatch;
    err_sharded <= 4 * err_ref + 2^-23 with err_ref that of the unsharded float32 device run, err_ref <= 1e-5."""
    s, args = sample_of(), update_args()
    truth = update64(s, args)
    ref = nets()
    policy.ppo_update(*ref, s, args)
    samples = shards_of(s)
    reps = [nets() for _ in range(2)]
    SL.Lockstep(2).run(lambda r, sh: policy.ppo_update(*reps[r], samples[r], args, shards=sh))
    torch.cuda.synchronize()
    e_ref, e_dev = everything(*ref), everything(*reps[0])
    assert sorted(truth) == sorted(e_ref) == sorted(e_dev)
    worst = {}
    for k in truth:
        if k.endswith(".step"):
            assert float(e_dev[k]) == float(truth[k]) == 1.0
            continue
        a, b = HL.err(e_ref[k], truth[k]), HL.err(e_dev[k], truth[k])
        worst[k] = (a, b)
    top = sorted(worst, key=lambda k: -worst[k][1])[:5]
    for k in top:
        print("%-50s err_ref %.3g err_sharded %.3g bound %.3g" % (k, worst[k][0], worst[k][1], HL.bound(worst[k][0])))
    for k, (a, b) in worst.items():
        assert a <= OL.CAP and b <= HL.bound(a), (k, a, b)


def _buffer(seed, T=2):
    from gmpe.engine import GmpeEngine
    from gmpe.rollout import DeviceRolloutBuffer
    cfg = gmpe.make_config(num_envs=N, num_agents=A, episode_length=5, seed=seed)
    eng = GmpeEngine(cfg, device=0)
    bargs = types.SimpleNamespace(gamma=0.99, gae_lambda=0.95, use_gae=True, use_proper_time_limits=False, use_valuenorm=False, use_popart=False)
    buf = DeviceRolloutBuffer(eng, T, use_centralized_V=False, policy_fields="all", learner_fields="all", args=bargs, recurrent_N=1, hidden_size=64)
    buf.warmup()
    g = torch.Generator(device=DEV)
    g.manual_seed(seed + 4)
    for t in range(T):
        logits = torch.randn((N * A, int(cfg.n_actions)), generator=g, device=DEV)
        vals = torch.randn((N * A, 1), generator=g, device=DEV)
        rnn = torch.rand((N * A, 1, 64), generator=g, device=DEV) * 2 - 1
        buf.act_step(logits, vals, rnn_states=rnn, rnn_states_critic=rnn)
    buf.compute_returns(torch.randn((N, A, 1), generator=g, device=DEV))
    return cfg, eng, buf


def test_train_with_shards_waits_for_nothing_and_the_replicas_stay_equal():
    """two replicas, each with a two-step buffer of its own, on two threads; torch's sync debug mode raises at every call that waits for the device"""
    made = [_buffer(13), _buffer(29)]
    args = _train_args(True)
    args.data_chunk_length = 2
    reps = [_train_nets(cfg, eng) for cfg, eng, _ in made]
    run = lambda x: x.run(lambda r, sh: policy.train(*reps[r], made[r][2], args, perms=["device"] * 2, shards=sh))
    run(SL.Lockstep(2))                                     # warm: every kernel loaded, every state created
    one = torch.ones((), device=DEV)
    torch.cuda.synchronize()
    x = SL.Lockstep(2)
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            one.item()
        infos = run(x)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert x.calls == [1 + 3 * 4] * 2                       # the advantages' statistics, then three exchanges per minibatch
    assert list(infos[0]) == list(policy.TRAIN_INFO)
    for k in policy.TRAIN_INFO:
        v = infos[0][k]
        assert v.dim() == 0 and v.dtype == torch.float32 and bool(torch.isfinite(v)) and same(v, infos[1][k]), k
    equal_dicts(everything(*reps[0]), everything(*reps[1]))
    assert all(float(st["step"]) == 8 for rep in reps for opt in rep[2:] for st in opt.state.values())
    for _, eng, _ in made:
        eng.check_errors()
        eng.close()


def test_popart_with_shards_is_ppo_losses_poparts_refusal():
    s, args = sample_of(), update_args(use_popart=True)
    x = SL.Lockstep(1)
    with pytest.raises(NotImplementedError, match="the PopArt variant has no sharded form"):
        policy.ppo_update(*nets(True), s, args, shards=x.rank(0))
    assert x.calls == [0]
