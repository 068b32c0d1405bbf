"""The rollout half of the action head on the device (include/gmpe.h gmpe_act_sample, gmpe.sample_actions) against the float64 restatement of
tests/act_lib.py (pinned to the reference's own run by tests/test_act_host.py), against that run itself (tests/golden/act_head.npz), and against
gmpe.ppo_losses, whose action_log_probs the stored ones must equal bit for bit.

Bounds: a sampled action equals the float64 restatement's on every row whose draw is not within (K + 4) * 2**-23 of a float64 CDF boundary; such an
ambiguous row takes one of the two actions next to its boundary, and at most 0.5 % of the rows are ambiguous (the host suite shows the float32
restatement inside the same bounds). Log-probs at the device's own actions: ppo_loss_lib.C_DEV = 160 units of U * (1 + |x|) against float64."""
import ctypes as C
import os

import numpy as np
import pytest

import gmpe
import act_lib as AL
import ppo_loss_lib as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "act_head.npz")
_REF = {}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64, 1: np.uint8}[a.itemsize])


def _offset(torch, a, off):
    """`a` on the device at `off` elements past a 256-byte aligned base: off 0 takes the 16-byte path, 1 the 4-byte one."""
    a = np.ascontiguousarray(a)
    buf = torch.empty(a.size + 8, dtype=torch.from_numpy(a).dtype, device="cuda")
    v = buf[off:off + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == (off * a.itemsize) % 16
    return v


def _ref(case):
    """The inputs of a case, its draws and the float64 restatement, computed once and shared."""
    if case not in _REF:
        fam, B, K, A, base, kind = case
        logits, avail = AL.family(fam, B, K, seed=0, avail=kind)
        u = AL.draws(AL.SEED, base, A, AL.DRAW, B)
        _REF[case] = (logits, avail, u, AL.restate(logits, avail, u, np.float64))
    return _REF[case]


def _sample(torch, logits, avail, A, base, draw=AL.DRAW, off=0, **kw):
    lg = _offset(torch, logits, off)
    av = None if avail is None else _offset(torch, avail, off)
    idx, act, lp = gmpe.sample_actions(lg, av, seed=AL.SEED, env_id_base=base, num_agents=A, draw=draw, **kw)
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (len(logits),) and act.dtype == torch.int64 and tuple(act.shape) == (len(logits), 1)
    assert lp.dtype == torch.float32 and tuple(lp.shape) == (len(logits), 1)
    assert torch.equal(idx.long(), act[:, 0])
    return idx.cpu().numpy(), lp.cpu().numpy()[:, 0]


IDS = lambda c: "%s-%dx%d-A%d-%s" % (c[0], c[1], c[2], c[3], c[5])


@pytest.mark.parametrize("case", AL.CASES, ids=IDS)
def test_sampled_actions_and_log_probs_against_float64_and_the_loss_kernel(case):
    import torch
    fam, B, K, A, base, kind = case
    logits, avail, u, r64 = _ref(case)
    a, lp = _sample(torch, logits, avail, A, base)
    R = np.arange(B)
    # ---- actions: the float64 action off the boundaries, one of the two neighbours at one
    amb, allowed = AL.ambiguity(r64, u, K)
    print("ambiguous rows %d of %d; rows that differ from float64: %d" % (amb.sum(), B, (a != r64["actions"]).sum()))
    assert amb.sum() <= AL.AMBIGUOUS_MAX * B
    assert (a[~amb] == r64["actions"][~amb]).all()
    assert allowed[R, a].all()
    if avail is not None:
        some = avail.any(axis=1)
        assert (avail[R, a][some] != 0).all()                                   # never an unavailable action
        stop = (avail.sum(axis=1) == 1)
        assert (stop.any() or B < 5) and (a[stop] == np.argmax(avail[stop], axis=1)).all() and (bits(lp[stop]) == 0).all()     # the only action, log-prob +0
    # ---- log-probs at the device's own actions against float64
    e = float(P.row_err(lp, r64["l"][R, a]).max())
    print("log-probs: %.1f units of U * (1 + |x|) (bound %.0f)" % (e, P.C_DEV))
    assert e <= P.C_DEV
    # ---- and bit for bit what the loss kernel recomputes: the importance weights of an unchanged policy are exactly 1
    z = lambda: torch.zeros(B, 1, device="cuda")
    f = dict(actions=torch.from_numpy(a.astype(np.int64)).cuda().view(B, 1), value_preds=z(), returns=z(), active_masks=torch.ones(B, 1, device="cuda"),
             old_action_log_probs=torch.from_numpy(lp).cuda().view(B, 1), adv_targ=z(),
             available_actions=None if avail is None else torch.from_numpy(avail).cuda())
    res = gmpe.ppo_losses(torch.from_numpy(logits).cuda(), z(), f, _Args())
    assert np.array_equal(bits(res.action_log_probs.cpu().numpy()[:, 0]), bits(lp))
    assert (res.imp_weights.cpu().numpy() == 1.0).all()


class _Args(object):
    clip_param, huber_delta, entropy_coef = 0.25, 10.0, 0.01
    use_policy_active_masks = use_value_active_masks = use_clipped_value_loss = use_huber_loss = True
    use_valuenorm = use_popart = False


def test_four_byte_path_gives_the_same_bits():
    import torch
    for case in (AL.CASES[1], AL.CASES[5]):                                     # K odd (the LDS image is the global one) and K even
        fam, B, K, A, base, kind = case
        logits, avail, u, r64 = _ref(case)
        a0, lp0 = _sample(torch, logits, avail, A, base, off=0)
        a1, lp1 = _sample(torch, logits, avail, A, base, off=1)
        assert np.array_equal(a0, a1) and np.array_equal(bits(lp0), bits(lp1))


@pytest.mark.parametrize("name", ("a", "b", "c", "d", "e", "f"))
def test_deterministic_mode_is_the_reference_mode(name):
    import torch
    d = np.load(GOLD)
    logits, avail = d[name + "_logits"], (d[name + "_avail"] if bool(d[name + "_has_avail"]) else None)
    a, lp = _sample(torch, logits, avail, 3, 0, deterministic=True)
    np.testing.assert_array_equal(a, d[name + "_mode"][:, 0])
    r64 = AL.restate(logits, avail, None, np.float64)
    assert float(P.row_err(lp, r64["mode_log_probs"]).max()) <= P.C_DEV
    a2, lp2 = _sample(torch, logits, avail, 10, 99, draw=7, deterministic=True)  # no draw enters
    assert np.array_equal(a, a2) and np.array_equal(bits(lp), bits(lp2))


def test_deterministic_mode_takes_the_first_index_on_exact_ties():
    import torch
    rng = np.random.RandomState(11)
    B, K = 300, 25
    logits = (rng.randint(-3, 4, (B, K)) * 0.5).astype(np.float32)             # few distinct values: the largest one repeats in most rows
    avail = (rng.rand(B, K) < 0.6).astype(np.float32)
    avail[np.arange(B), rng.randint(0, K, B)] = 1.0
    avail[::9] = 0.0                                                            # nothing available: the uniform row, mode 0
    for av in (None, avail):
        want = AL.restate(logits, av, None, np.float64)["mode"]
        x = logits if av is None else np.where(av != 0, logits, -np.inf)
        ties = ((x == x.max(axis=1, keepdims=True)).sum(axis=1) > 1)
        assert ties.mean() > 0.5
        a, _ = _sample(torch, logits, av, 3, 0, deterministic=True)
        np.testing.assert_array_equal(a, want)
        if av is not None:
            assert (a[::9] == 0).all() and (av[np.arange(B), a][av.any(axis=1)] != 0).all()


def test_dones_path_equals_the_explicit_availability():
    import torch
    for K, B in ((25, 1030), (64, 257), (1, 63)):
        rng = np.random.RandomState(K)
        logits, _ = AL.family("wide", B, K, seed=4, avail="none")
        dones = (rng.rand(B) < 0.4).astype(np.uint8)
        avail = np.ones((B, K), np.float32)
        avail[dones != 0] = 0.0
        avail[dones != 0, K // 2] = 1.0
        a0, lp0 = _sample(torch, logits, avail, 10, 3)
        a1, lp1 = _sample(torch, logits, None, 10, 3, dones_prev=torch.from_numpy(dones).cuda())
        a2, lp2 = _sample(torch, logits, None, 10, 3, dones_prev=torch.from_numpy(dones).cuda().bool(), stop_action=K // 2)
        assert np.array_equal(a0, a1) and np.array_equal(bits(lp0), bits(lp1)) and np.array_equal(a0, a2) and np.array_equal(bits(lp0), bits(lp2))
        assert (a1[dones != 0] == K // 2).all() and (bits(lp1[dones != 0]) == 0).all()
        if K > 1:
            assert (a1[dones == 0] != K // 2).any()
            stop = 0
            a3, _ = _sample(torch, logits, None, 10, 3, dones_prev=torch.from_numpy(dones).cuda(), stop_action=stop)
            assert (a3[dones != 0] == stop).all()


def test_actions_do_not_depend_on_how_the_envs_are_batched():
    import torch
    N, A, K, base = 104, 10, 25, 1000                                           # 1040 rows: five tiles, env boundaries inside tiles
    logits, avail = AL.family("unit", N * A, K, seed=8, avail="mixed")
    whole = _sample(torch, logits, avail, A, base)

    def parts(cuts):
        out = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            out.append(_sample(torch, logits[lo * A:hi * A], avail[lo * A:hi * A], A, base + lo))
        return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])
    for cuts in ((0, N // 2, N), (0, 1, 30, 31, 77, N)):                        # two halves; an uneven composition with single-env calls
        a, lp = parts(cuts)
        assert np.array_equal(a, whole[0]) and np.array_equal(bits(lp), bits(whole[1]))
    # the key is the env's global id, not the row: the same rows under another env_id_base draw other numbers
    other = _sample(torch, logits, avail, A, base + 1)
    assert not np.array_equal(other[0], whole[0])
    u = AL.draws(AL.SEED, base, A, AL.DRAW, N * A)
    r64 = AL.restate(logits, avail, u, np.float64)
    amb, allowed = AL.ambiguity(r64, u, K)
    assert (whole[0][~amb] == r64["actions"][~amb]).all() and allowed[np.arange(N * A), whole[0]].all()


def test_draw_changes_the_actions_and_the_device_counter_counts():
    import torch
    B, K, A, base, d0 = 257, 25, 3, 5, 1 << 40
    logits, avail = AL.family("unit", B, K, seed=9, avail="mixed")
    host = [_sample(torch, logits, avail, A, base, draw=d0 + i) for i in range(3)]
    assert not np.array_equal(host[0][0], host[1][0]) and not np.array_equal(host[1][0], host[2][0])
    for i in range(2):                                                          # and each is the restatement's for its draw
        u = AL.draws(AL.SEED, base, A, d0 + i, B)
        r64 = AL.restate(logits, avail, u, np.float64)
        amb, allowed = AL.ambiguity(r64, u, K)
        assert (host[i][0][~amb] == r64["actions"][~amb]).all() and allowed[np.arange(B), host[i][0]].all()
    ctr = torch.tensor([d0], dtype=torch.int64, device="cuda")
    for i in range(2):
        a, lp = _sample(torch, logits, avail, A, base, draw=0, draw_dev=ctr)
        assert np.array_equal(a, host[i][0]) and np.array_equal(bits(lp), bits(host[i][1]))
    assert int(ctr.item()) == d0 + 2
    a, _ = _sample(torch, logits, avail, A, base, draw=1, draw_dev=ctr, draw_inc=5)        # *draw_dev + draw
    u = AL.draws(AL.SEED, base, A, d0 + 3, B)
    r64 = AL.restate(logits, avail, u, np.float64)
    amb, _ = AL.ambiguity(r64, u, K)
    assert (a[~amb] == r64["actions"][~amb]).all() and int(ctr.item()) == d0 + 7


def test_a_captured_chain_of_two_calls_draws_fresh_numbers_at_every_replay():
    import torch
    B, K, A, base, d0 = 300, 25, 3, 0, 77
    logits, avail = AL.family("unit", B, K, seed=10, avail="mixed")
    lg, av = torch.from_numpy(logits).cuda(), torch.from_numpy(avail).cuda()
    host = [_sample(torch, logits, avail, A, base, draw=d0 + i) for i in range(4)]
    assert len({h[0].tobytes() for h in host}) == 4
    ctr = torch.tensor([d0], dtype=torch.int64, device="cuda")
    outs = [dict(action_idx=torch.zeros(B, dtype=torch.int32, device="cuda"), actions=torch.zeros(B, 1, dtype=torch.int64, device="cuda"),
                 actions_f32=torch.zeros(B, 1, device="cuda"), action_log_probs=torch.zeros(B, 1, device="cuda")) for _ in range(2)]

    def chain():
        for o in outs:
            gmpe.sample_actions(lg, av, seed=AL.SEED, env_id_base=base, num_agents=A, draw=0, draw_dev=ctr, out=o)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        chain()                                                                 # warm-up on a side stream, as torch.cuda.graph wants
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    ctr.fill_(d0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                               # one stream, a linear chain: no parallel branches
        chain()
    for rep in range(2):
        for o in outs:
            for t in o.values():
                t.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        for i, o in enumerate(outs):
            want = host[2 * rep + i]
            assert np.array_equal(o["action_idx"].cpu().numpy(), want[0]), (rep, i)
            assert np.array_equal(bits(o["action_log_probs"].cpu().numpy()[:, 0]), bits(want[1])), (rep, i)
            assert np.array_equal(o["actions"].cpu().numpy()[:, 0], want[0]) and np.array_equal(o["actions_f32"].cpu().numpy()[:, 0], want[0].astype(np.float32))
    assert int(ctr.item()) == d0 + 4


def test_half_precision_logits_are_widened_and_bad_plans_launch_nothing():
    import torch
    from gmpe import _lib
    B, K, A = 63, 5, 3
    logits, avail = AL.family("unit", B, K, seed=12, avail="mixed")
    h = torch.from_numpy(logits).cuda().half()
    a0, lp0 = _sample(torch, h.float().cpu().numpy(), avail, A, 0)
    idx, act, lp = gmpe.sample_actions(h, torch.from_numpy(avail).cuda(), seed=AL.SEED, num_agents=A, draw=AL.DRAW)
    assert np.array_equal(idx.cpu().numpy(), a0) and np.array_equal(bits(lp.cpu().numpy()[:, 0]), bits(lp0))
    # a refused plan writes nothing
    lg = torch.from_numpy(logits).cuda()
    out_idx = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    out_lp = torch.full((B,), -7.0, device="cuda")
    plan = _lib.GmpeActPlan()
    plan.rows, plan.n_actions, plan.num_agents, plan.stop_action = B, K, A, K        # stop_action out of range
    plan.logits, plan.action_idx, plan.log_probs = lg.data_ptr(), out_idx.data_ptr(), out_lp.data_ptr()
    lib = _lib.load()
    assert lib.gmpe_act_sample(0, C.byref(plan), None) == -1 and b"stop_action" in lib.gmpe_last_error()
    plan.stop_action, plan.reserved = 0, 3
    assert lib.gmpe_act_sample(0, C.byref(plan), None) == -1 and b"reserved" in lib.gmpe_last_error()
    torch.cuda.synchronize()
    assert (out_idx == -7).all() and (out_lp == -7.0).all()
    with pytest.raises(ValueError, match="must be on"):
        gmpe.sample_actions(lg, torch.ones(B, K), seed=1, num_agents=A, draw=0)
