"""The policy's action head on the device (gmpe.action_logits / gmpe.act_head, gmpe_head_forward / gmpe_head_backward / gmpe_act_head) against the float64
formulas of tests/head_lib.py. err(a) = max|a - a64| / max(1, max|a64|); per array the device is held to err_dev <= 4 * err_ref + 2^-23, err_ref being the
error of the same formulas in float32 torch on the CPU, capped at 1e-5. Everything that is claimed bit for bit is compared bit for bit: a row's logits and
grad_features whatever its batch, the fused rollout launch against forward + sample_actions, and the importance weights of an unchanged policy, which are
exactly 1 from a rollout of one shape to a minibatch of another."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

import gmpe
import head_lib as HL
from gmpe import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                                              # bytes behind the workspace and behind every output, which the kernels must leave alone
NAN = float("nan")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).reshape(-1).view(np.uint32)


def same(a, b):
    return np.asarray(a).shape == np.asarray(b).shape and np.array_equal(bits(a), bits(b))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def offset(a, off):
    """`a` on the device at `off` elements past an aligned base: off 0 takes the 16-byte path, 1 the 4-byte one"""
    a = np.ascontiguousarray(a)
    buf = torch.empty(a.size + 8, dtype=torch.from_numpy(a).dtype, device=DEV)
    v = buf[off:off + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == (off * a.itemsize) % 16
    return v


@functools.lru_cache(maxsize=None)
def device_act(K, source):
    return HL.act_layer(K, source, DEV)


def run(f, act, g, workspace=None):
    """gmpe.action_logits + autograd with grad_logits g -> the four arrays of head_lib.ARRAYS"""
    lin = act.action_out.linear
    ft = (f if isinstance(f, torch.Tensor) else dev(f)).detach().requires_grad_(True)
    gt = g if isinstance(g, torch.Tensor) else dev(g)
    logits = gmpe.action_logits(ft, act, workspace=workspace)
    gf, gw, gb = torch.autograd.grad(logits, [ft, lin.weight, lin.bias], grad_outputs=gt)
    torch.cuda.synchronize()
    return dict(logits=logits.detach().cpu().numpy(), grad_features=gf.cpu().numpy(), grad_weight=gw.cpu().numpy(), grad_bias=gb.cpu().numpy())


@functools.lru_cache(maxsize=None)
def device_run(case):
    rows, K, source = case
    f, w, b, g, _, _ = HL.truth(case)
    return run(f, device_act(K, source), g)


def check(got, t64, e_ref, what):
    worst = 0.0
    for k in HL.ARRAYS:
        e_dev = HL.err(got[k], t64[k])
        worst = max(worst, e_dev / HL.bound(e_ref[k]))
        print("%s %-14s err_ref %.3g err_dev %.3g bound %.3g ratio %.3f" % (what, k, e_ref[k], e_dev, HL.bound(e_ref[k]), e_dev / HL.bound(e_ref[k])))
    for k in HL.ARRAYS:
        assert e_ref[k] <= HL.CAP, (what, k, e_ref[k])
        assert HL.err(got[k], t64[k]) <= HL.bound(e_ref[k]), (what, k, HL.err(got[k], t64[k]), e_ref[k])
    return worst


def loss_args(**over):
    kw = dict(clip_param=0.2, huber_delta=10.0, entropy_coef=0.01, use_policy_active_masks=True, use_value_active_masks=True, use_clipped_value_loss=True,
              use_huber_loss=True, use_valuenorm=False, use_popart=False)
    kw.update(over)
    return types.SimpleNamespace(**kw)


def fields(rows, K, seed=0, actions=None, old_lp=None, avail=None):
    """the columns of a minibatch as ppo_losses takes them, random where not given"""
    rng = np.random.RandomState(900 + rows + 17 * K + seed)
    f32 = np.float32
    d = dict(actions=rng.randint(0, K, (rows, 1)).astype(np.int64) if actions is None else actions,
             value_preds=rng.randn(rows, 1).astype(f32), returns=rng.randn(rows, 1).astype(f32),
             active_masks=(rng.rand(rows, 1) > 0.1).astype(f32), old_action_log_probs=(-rng.rand(rows, 1) * 3).astype(f32) if old_lp is None else old_lp,
             adv_targ=rng.randn(rows, 1).astype(f32))
    d = {k: v if isinstance(v, torch.Tensor) else dev(v) for k, v in d.items()}
    if avail is not None:
        d["available_actions"] = avail
    return d, dev(rng.randn(rows, 1).astype(f32))


# ---------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("case", HL.CASES, ids=HL.case_id)
def test_forward_and_backward_agree_with_float64(case):
    f, w, b, g, t64, e_ref = HL.truth(case)
    check(device_run(case), t64, e_ref, HL.case_id(case))


@pytest.mark.parametrize("case", [(513, 25, "actor"), (257, 5, "random"), (4097, 64, "random")], ids=HL.case_id)
def test_backward_of_the_gradient_ppo_losses_produced(case):
    """grad_logits as the loss kernels leave it (small: of the order 1 / rows); the truth is formed from the same array, which isolates the head"""
    rows, K, source = case
    f, w, b, _, _, _ = HL.truth(case)
    act = device_act(K, source)
    with torch.no_grad():
        lg = gmpe.action_logits(dev(f), act)
    lg.requires_grad_(True)
    fl, values = fields(rows, K)
    gmpe.ppo_losses(lg, values, fl, loss_args()).actor_loss.backward()
    g = lg.grad
    gh = g.cpu().numpy()
    assert np.abs(gh).max() > 0
    t64, e_ref = HL.truth_of(f, w, b, gh)
    check(run(f, act, g), t64, e_ref, HL.case_id(case) + " ppo_losses' gradient")


# ---------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("K", [24, 25])
def test_a_row_does_not_depend_on_its_batch_or_its_place(K):
    case = (513, K, "random")
    f, w, b, g, _, _ = HL.truth(case)
    act = device_act(K, "random")
    full = device_run(case)
    for n in (1, 5):
        part = run(f[:n], act, g[:n])
        mid = run(f[300:300 + n], act, g[300:300 + n])
        for k in ("logits", "grad_features"):
            assert same(part[k], full[k][:n]) and same(mid[k], full[k][300:300 + n]), (n, k)
    rev = run(f[::-1], act, g[::-1])
    for k in ("logits", "grad_features"):
        assert same(rev[k][::-1], full[k]), k


def test_two_backward_calls_agree_and_a_reused_workspace_does_not_show():
    case = (4097, 25, "actor")
    f, w, b, g, _, _ = HL.truth(case)
    act = device_act(25, "actor")
    ws = torch.full((gmpe.head_workspace_bytes(4097, 25) + 24,), 0xA5, dtype=torch.uint8, device=DEV)
    a, c = device_run(case), run(f, act, g, workspace=ws)
    d = run(f, act, g, workspace=ws)
    for k in HL.ARRAYS:
        assert same(a[k], c[k]) and same(a[k], d[k]), k
    with pytest.raises(ValueError, match="workspace must be a contiguous uint8 tensor of at least"):
        run(f, act, g, workspace=ws[:1000])


def test_the_last_of_4097_rows_alone_gives_the_one_row_calls_parameter_gradients():
    """partition(4097) = 128 parts of 33 rows, 17 tiles: with grad_logits zero except in the last row every other row adds exact zeros to the double sums,
    so grad_weight and grad_bias have the bits of the one-row call"""
    for K in (25, 64):
        f, w, b, g, _, _ = HL.truth((4097, K, "random"))
        act = device_act(K, "random")
        g1 = np.zeros_like(g)
        g1[-1] = g[-1]
        many, one = run(f, act, g1), run(f[-1:], act, g[-1:])
        assert np.abs(one["grad_weight"]).max() > 0 and np.abs(one["grad_bias"]).max() > 0
        assert same(many["grad_weight"], one["grad_weight"]) and same(many["grad_bias"], one["grad_bias"])
        assert same(many["grad_features"][-1:], one["grad_features"]) and not many["grad_features"][:-1].any()


# ---------------------------------------------------------------------------------------------- 6 (the C entries; used by 2's unaligned test too)
def guarded(n, dtype=torch.float32, fill=NAN, off=0):
    """n elements with GUARD bytes behind them -> (the whole buffer, the view the kernel gets)"""
    extra = GUARD // torch.empty((), dtype=dtype).element_size()
    buf = torch.full((n + extra + 8,), fill, dtype=dtype, device=DEV)
    return buf, buf[off:off + n]


def untouched(buf, n, off=0, fill=NAN):
    tail = buf[off + n:].cpu().numpy()
    head = buf[:off].cpu().numpy()
    ok = (lambda a: np.isnan(a).all()) if fill != fill else (lambda a: (a == fill).all())
    return ok(tail) and ok(head)


def c_call(case, off=0, fill=0, stream=None, backward=True):
    """gmpe_head_forward (+ gmpe_head_backward, twice) through ctypes with caller-owned buffers at `off` floats past an aligned base: one offset for every
    pointer, or a dict {plan field: offset} with the fields it does not name at 0"""
    lib = _lib.load()
    rows, K, source = case
    f, w, b, g, _, _ = HL.truth(case)
    o = (lambda k: off.get(k, 0)) if isinstance(off, dict) else (lambda k: off)
    fd, wd, bd, gd = offset(f, o("features")), offset(w, o("weight")), offset(b, o("bias")), offset(g, o("grad_logits"))
    st = C.c_void_p((stream or torch.cuda.current_stream(torch.device(DEV))).cuda_stream)
    p = _lib.GmpeHeadPlan()
    p.rows, p.n_actions, p.hidden = rows, K, 64
    p.features, p.weight, p.bias = fd.data_ptr(), wd.data_ptr(), bd.data_ptr()
    lbuf, lg = guarded(rows * K, off=o("logits_out"))
    p.logits_out = lg.data_ptr()
    _lib.check(lib.gmpe_head_forward(0, C.byref(p), st), "gmpe_head_forward")
    torch.cuda.synchronize()
    assert untouched(lbuf, rows * K, o("logits_out")), "logits_out: written outside"
    res = {"logits": lg.cpu().numpy().reshape(rows, K)}
    if backward:
        nbytes = gmpe.head_workspace_bytes(rows, K)
        ws = torch.full((nbytes + GUARD,), fill, dtype=torch.uint8, device=DEV)
        outs = {k: guarded(n, off=o(k)) for k, n in (("grad_features", rows * 64), ("grad_weight", K * 64), ("grad_bias", K))}
        p.logits_out, p.bias, p.grad_logits = None, None, gd.data_ptr()                # backward reads neither
        for k, (_, v) in outs.items():
            setattr(p, k, v.data_ptr())
        p.workspace, p.workspace_bytes = ws.data_ptr(), nbytes
        first = None
        for rep in range(2):                            # backward may be repeated on one plan: fresh outputs, the same bits
            _lib.check(lib.gmpe_head_backward(0, C.byref(p), st), "gmpe_head_backward")
            torch.cuda.synchronize()
            if rep == 0:
                first = {k: v.clone() for k, (_, v) in outs.items()}
                for _, v in outs.values():
                    v.fill_(NAN)
                torch.cuda.synchronize()
        assert bool((ws[nbytes:] == fill).all()), "bytes past the workspace were written"
        for k, (buf, v) in outs.items():
            assert untouched(buf, v.numel(), o(k)), k + ": written outside"
            assert same(v.cpu().numpy(), first[k].cpu().numpy()), "the second backward call differs: " + k
            res[k] = v.cpu().numpy().reshape(dict(grad_features=(rows, 64), grad_weight=(K, 64), grad_bias=(K,))[k])
    return res


@pytest.mark.parametrize("case", [(513, 25, "actor"), (257, 24, "random"), (4097, 64, "random"), (65, 1, "random")], ids=HL.case_id)
def test_the_c_entries_give_the_wrappers_bits_aligned_or_not_and_stay_inside_their_outputs(case):
    a = device_run(case)
    for off in (0, 1):
        b = c_call(case, off=off)
        assert sorted(a) == sorted(b)
        for k in a:
            assert same(a[k], b[k]), (off, k)


def test_each_alignment_flag_alone_gives_the_same_bits():
    """gmpe_head.hip chooses 16-byte or 4-byte units per array — features, weight, grad_features, and the [rows, K] array of the call (logits_out forward,
    grad_logits backward) — where one offset for all pointers only ever runs all four together: each one off on its own, and features aligned while both
    of backward's other row arrays are off"""
    case = (257, 25, "actor")
    a = device_run(case)
    for off in ({"features": 1}, {"weight": 1}, {"grad_features": 1}, {"logits_out": 1, "grad_logits": 1}, {"grad_features": 1, "grad_logits": 1}):
        b = c_call(case, off=off)
        assert sorted(a) == sorted(b)
        for k in a:
            assert same(a[k], b[k]), (off, k)


def test_the_workspaces_old_contents_do_not_show_and_a_side_stream_works():
    case = (513, 25, "actor")
    full = device_run(case)
    zeros, ones = c_call(case, fill=0x00), c_call(case, fill=0xFF)
    fwd = c_call(case, backward=False)
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        other = c_call(case, stream=side)
        f, w, b, g, _, _ = HL.truth(case)
        wrapped = run(f, device_act(25, "actor"), g)                                # the wrapper launches on the current stream
    for k in full:
        assert same(zeros[k], full[k]) and same(ones[k], full[k]) and same(other[k], full[k]) and same(wrapped[k], full[k]), k
    assert same(fwd["logits"], full["logits"])


def test_each_backward_output_may_be_left_out():
    lib = _lib.load()
    case = (257, 5, "random")
    rows, K, _ = case
    f, w, b, g, _, _ = HL.truth(case)
    full = device_run(case)
    fd, wd, gd = dev(f), dev(w), dev(g)
    ws = torch.empty((gmpe.head_workspace_bytes(rows, K),), dtype=torch.uint8, device=DEV)
    shapes = dict(grad_features=(rows, 64), grad_weight=(K, 64), grad_bias=(K,))
    for keep in shapes:
        p = _lib.GmpeHeadPlan()
        p.rows, p.n_actions, p.hidden = rows, K, 64
        p.features, p.weight, p.grad_logits = fd.data_ptr(), wd.data_ptr(), gd.data_ptr()
        p.workspace, p.workspace_bytes = ws.data_ptr(), ws.numel()
        out = torch.full(shapes[keep], NAN, device=DEV)
        setattr(p, keep, out.data_ptr())
        _lib.check(lib.gmpe_head_backward(0, C.byref(p), C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)), "gmpe_head_backward")
        torch.cuda.synchronize()
        assert same(out.cpu().numpy(), full[keep]), keep


# ---------------------------------------------------------------------------------------------- 3
def availability(rows, K, seed=0):
    rng = np.random.RandomState(300 + rows + K + seed)
    av = (rng.rand(rows, K) > 0.4).astype(np.float32)
    av[np.arange(rows), rng.randint(0, K, rows)] = 1.0                              # at least one available ...
    av[rows // 2] = 0.0                                                             # ... but for one row: the uniform row over all K
    return av, (rng.rand(rows) > 0.7).astype(np.uint8)


@pytest.mark.parametrize("K", HL.KS)
@pytest.mark.parametrize("rows", [257, 513])
def test_the_fused_launch_equals_forward_then_sample_actions(rows, K):
    f, w, b, _, _, _ = HL.truth((rows, K, "random"))
    act = device_act(K, "random")
    fd = dev(f)
    av, dn = availability(rows, K)
    with torch.no_grad():
        lg = gmpe.action_logits(fd, act)
    sources = (dict(), dict(available_actions=dev(av)), dict(dones_prev=dev(dn)), dict(dones_prev=dev(dn), stop_action=K - 1))
    n = 0
    for src in sources:
        for det in (False, True):
            kw = dict(seed=12345, env_id_base=3, num_agents=7, draw=11 + n, deterministic=det, **src)
            want = gmpe.sample_actions(lg, **kw)
            got = gmpe.act_head(fd, act, **kw)
            torch.cuda.synchronize()
            for a, c, name in zip(got, want, ("action_idx", "actions", "action_log_probs")):
                assert a.dtype == c.dtype and a.shape == c.shape and torch.equal(a, c) and same(a.float().cpu().numpy(), c.float().cpu().numpy()), (src.keys(), det, name)
            n += 1
    # out= views into larger buffers, the logits among them; the rest of the buffers stays as it was
    big = {k: torch.full((3, rows), -7, dtype=dt, device=DEV) for k, dt in (("action_idx", torch.int32), ("actions", torch.int64), ("actions_f32", torch.float32),
                                                                            ("action_log_probs", torch.float32))}
    lbig = torch.full((3, rows, K), -7.0, device=DEV)
    out = {k: v[1] for k, v in big.items()}
    kw = dict(seed=5, num_agents=3, draw=2, available_actions=dev(av))
    want = gmpe.sample_actions(lg, out={k: torch.empty_like(v) for k, v in out.items()}, **kw)
    got = gmpe.act_head(fd, act, out=dict(out, logits=lbig[1]), **kw)
    torch.cuda.synchronize()
    assert got[0].data_ptr() == big["action_idx"][1].data_ptr() and got[1].data_ptr() == big["actions"][1].data_ptr()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(-1), want[1].view(-1)) and same(got[2].cpu().numpy().ravel(), want[2].cpu().numpy().ravel())
    assert torch.equal(big["actions_f32"][1], want[0].float()) and same(lbig[1].cpu().numpy(), lg.cpu().numpy())
    for v in list(big.values()) + [lbig]:
        assert bool((v[0] == -7).all()) and bool((v[2] == -7).all())
    unav = torch.gather(dev(av), 1, got[0].long().view(-1, 1)).view(-1) == 0
    unav[rows // 2] = False                                                         # the row with nothing available is sampled over all K
    assert not bool(unav.any())


# ---------------------------------------------------------------------------------------------- 4
def test_an_unchanged_policy_has_importance_weights_of_exactly_one_end_to_end():
    """a rollout step of 32 envs x 10 agents through act_head, then a permuted 130-row minibatch through action_logits and ppo_losses: the two batch
    shapes differ, the logits of a row do not"""
    rows, K, A = 320, 25, 10
    for source in ("actor", "rotate"):
        act = device_act(K, source)
        f = dev(HL.inputs(rows, K, seed=3)[0])
        av = dev(availability(rows, K)[0])
        idx, actions, logp = gmpe.act_head(f, act, av, seed=77, env_id_base=5, num_agents=A, draw=4)
        perm = torch.from_numpy(np.random.RandomState(1).permutation(rows)[:130].copy()).to(DEV)
        logits = gmpe.action_logits(f[perm].contiguous().requires_grad_(True), act)
        fl, values = fields(130, K, actions=actions[perm].contiguous(), old_lp=logp[perm].contiguous(), avail=av[perm].contiguous())
        res = gmpe.ppo_losses(logits, values, fl, loss_args())
        torch.cuda.synchronize()
        ratio = res.imp_weights.cpu().numpy()
        assert ratio.shape == (130, 1) and np.array_equal(bits(ratio), bits(np.ones((130, 1), np.float32))), source
        assert same(res.action_log_probs.cpu().numpy(), logp[perm].cpu().numpy()) and float(res.ratio_mean) == 1.0
        assert len(np.unique(idx.cpu().numpy())) > 5 and np.abs(logp.cpu().numpy()).max() > 0


# ---------------------------------------------------------------------------------------------- 5
def c_backward(f, w, g):
    lib = _lib.load()
    rows, K = g.shape
    ws = torch.empty((gmpe.head_workspace_bytes(rows, K),), dtype=torch.uint8, device=DEV)
    gf, gw, gb = torch.empty((rows, 64), device=DEV), torch.empty((K, 64), device=DEV), torch.empty((K,), device=DEV)
    p = _lib.GmpeHeadPlan()
    p.rows, p.n_actions, p.hidden = rows, K, 64
    p.features, p.weight, p.grad_logits = f.data_ptr(), w.data_ptr(), g.data_ptr()
    p.grad_features, p.grad_weight, p.grad_bias = gf.data_ptr(), gw.data_ptr(), gb.data_ptr()
    p.workspace, p.workspace_bytes = ws.data_ptr(), ws.numel()
    _lib.check(lib.gmpe_head_backward(0, C.byref(p), C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)), "gmpe_head_backward")
    torch.cuda.synchronize()
    return gf, gw, gb


def test_autograd_carries_the_loss_through_the_head(monkeypatch):
    """(actor_loss * 3).backward(): the gradient that reaches the head is the loss kernel's grad_logits times 3 (one float32 product per element, formed by
    autograd); weight.grad, bias.grad and actor_features.grad are the C entry's arrays for exactly that gradient"""
    rows, K = 513, 25
    act = HL.act_layer(K, "actor", DEV)
    lin = act.action_out.linear
    f = dev(HL.inputs(rows, K, seed=5)[0]).requires_grad_(True)
    fl, values = fields(rows, K)
    logits = gmpe.action_logits(f, act)
    assert logits.requires_grad and tuple(logits.shape) == (rows, K)
    leaf = logits.detach().clone().requires_grad_(True)
    (gmpe.ppo_losses(leaf, values, fl, loss_args()).actor_loss * 3).backward()
    (gmpe.ppo_losses(logits, values, fl, loss_args()).actor_loss * 3).backward()
    gf, gw, gb = c_backward(f.detach(), lin.weight.detach(), leaf.grad.contiguous())
    assert same(f.grad.cpu().numpy(), gf.cpu().numpy()) and same(lin.weight.grad.cpu().numpy(), gw.cpu().numpy()) and same(lin.bias.grad.cpu().numpy(), gb.cpu().numpy())
    g1 = (leaf.grad / 3).cpu().numpy()
    t64, _ = HL.truth_of(f.detach().cpu().numpy(), lin.weight.detach().cpu().numpy(), lin.bias.detach().cpu().numpy(), g1)
    for k, got in (("grad_features", gf), ("grad_weight", gw), ("grad_bias", gb)):       # ... and three times the gradients of the loss itself
        assert HL.err(got.cpu().numpy() / 3 * rows, t64[k] * rows) <= 1e-5, k
    # only what requires a gradient is formed
    lin.weight.grad = lin.bias.grad = None
    lg2 = gmpe.action_logits(f.detach(), act)
    lg2.sum().backward()
    assert lin.weight.grad is not None and same(lin.bias.grad.cpu().numpy(), np.full((K,), float(rows), np.float32))
    # under no_grad, or when nothing requires a gradient: the forward-only plan, no workspace, no node; the same bits
    def no_workspace(*a, **k):
        raise AssertionError("a forward-only call asked for a workspace")
    monkeypatch.setattr(gmpe.head, "head_workspace_bytes", no_workspace)
    with torch.no_grad():
        quiet = gmpe.action_logits(f, act)
    frozen = HL.act_layer(K, "actor", DEV).requires_grad_(False)
    cold = gmpe.action_logits(f.detach(), frozen)
    assert quiet.grad_fn is None and not quiet.requires_grad and cold.grad_fn is None
    assert same(quiet.cpu().numpy(), logits.detach().cpu().numpy()) and same(cold.cpu().numpy(), logits.detach().cpu().numpy())


class _World1(object):
    world, rank = 1, 0

    def exchange(self, local):
        return local.reshape(1, -1).clone()


def test_the_popart_and_the_sharded_loss_take_the_logits_unchanged():
    rows, K = 257, 25
    act = HL.act_layer(K, "rotate", DEV)
    lin = act.action_out.linear
    f = dev(HL.inputs(rows, K, seed=9)[0])
    fl, values = fields(rows, K)
    plain = gmpe.ppo_losses(gmpe.action_logits(f, act), values, fl, loss_args())
    plain.actor_loss.backward()
    want = lin.weight.grad.clone()
    lin.weight.grad = None
    sharded = gmpe.ppo_losses(gmpe.action_logits(f, act), values, fl, loss_args(), shards=_World1())
    sharded.actor_loss.backward()
    assert same(sharded.action_log_probs.cpu().numpy(), plain.action_log_probs.cpu().numpy())
    assert torch.allclose(lin.weight.grad, want, rtol=1e-5, atol=1e-8) and abs(float(sharded.actor_loss.detach()) - float(plain.actor_loss.detach())) <= 1e-6
    lin.weight.grad = None
    pa = HL.PopArt(DEV)
    w_obj = pa.weight
    pop = gmpe.ppo_losses_popart(gmpe.action_logits(f, act), dev(HL.inputs(rows, K, seed=10)[0]).requires_grad_(True), fl, loss_args(use_popart=True), pa)
    pop.actor_loss.backward()
    pop.value_loss.backward()
    torch.cuda.synchronize()
    assert same(pop.action_log_probs.cpu().numpy(), plain.action_log_probs.cpu().numpy())
    assert same(lin.weight.grad.cpu().numpy(), want.cpu().numpy()) and w_obj.grad is not None and bool(torch.isfinite(w_obj.grad).all())


# ---------------------------------------------------------------------------------------------- 6
def test_a_captured_act_head_draws_fresh_numbers_at_every_replay():
    rows, K, A = 513, 25, 9
    act = device_act(K, "actor")
    f = dev(HL.inputs(rows, K, seed=2)[0])
    av = dev(availability(rows, K)[0])
    kw = dict(seed=99, env_id_base=2, num_agents=A)
    want = [gmpe.act_head(f, act, av, draw=6 + i, **kw) for i in range(2)]
    assert not torch.equal(want[0][0], want[1][0])
    ctr = torch.full((1,), 6, dtype=torch.int64, device=DEV)
    out = {"action_idx": torch.empty(rows, dtype=torch.int32, device=DEV), "actions": torch.empty((rows, 1), dtype=torch.int64, device=DEV),
           "action_log_probs": torch.empty((rows, 1), device=DEV), "logits": torch.empty((rows, K), device=DEV)}
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        gmpe.act_head(f, act, av, draw=0, draw_dev=ctr, out=out, **kw)             # warm-up outside the capture (it raises the kernel's LDS limit once)
        ctr.fill_(6)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gmpe.act_head(f, act, av, draw=0, draw_dev=ctr, out=out, **kw)
    for i in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out["action_idx"], want[i][0]) and torch.equal(out["actions"], want[i][1]), i
        assert same(out["action_log_probs"].cpu().numpy(), want[i][2].cpu().numpy()), i
    assert int(ctr.item()) == 8
    with torch.no_grad():
        assert same(out["logits"].cpu().numpy(), gmpe.action_logits(f, act).cpu().numpy())
