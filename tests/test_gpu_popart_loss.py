"""The PPO loss with PopArt on the device (include/gmpe.h gmpe_ppo_loss_popart, gmpe.ppo_losses_popart) against the reference's own run
(tests/golden/popart_loss.npz) and the restatements of tests/popart_lib.py (pinned to that run by tests/test_popart_host.py).

How the comparison is cut (popart_lib): the value head's summation order is the device's choice, so
  * `values` are checked against float64 with the dot-product bound (H + 2) * U * (sum_j |F_rj * W_j| + |b|), which holds for any order;
  * everything after the head is compared with the float64 restatement evaluated AT the device's own values, fed the device's own PopArt tensors as they
    were before the call: per element C_DEV * U * (1 + |x|) with gradients multiplied back by their denominator (grad_features: C_ROW = C_DEV);
    grad_weight / grad_bias are exact double sums of exact products of the device's g_r, each of which carries C_DEV * U * (1 + |D g_r|) / D, so column j
    gets C_DEV * U * sum_r |F_rj| * (1 + |D g_r|) / D (+ one float32 rounding); the scalars (C_DEV + 2) * U * sum|term| / denominator;
  * mean, mean_sq, debiasing_term within the float32 summation noise of the batch means, (log2(B) + 4) * U * mean|x|; stddev', W', b' within
    C_LAYER * U * (1 + |x|) of the float64 rescale fed the device's own statistics (the bias bound carries the cancellation, popart_lib.layer_bounds).
On `exact` the first minibatch is bit for bit against the reference's arrays. From the second minibatch on the rescaled weights are no longer short, a
float32 dot product rounds and its bits depend on the order of the sum: there the six PopArt tensors (which do not depend on the values) stay bit for bit
against the reference, the values get the dot-product bound and grad_features must be the bits of the float32 restatement at the device's own values."""
import os
import types

import numpy as np
import pytest

import gmpe
import popart_lib as PL
import ppo_loss_lib as P
from test_popart_host import GOLD, bits, fixture_case

pytestmark = pytest.mark.gpu
_REF = {}


def _report(what, got, want):
    """Print how two float32 arrays differ before a bitwise assertion: elements whose bits differ, those that differ in the sign of a zero only, and the
    largest difference in units of the last place."""
    g, w = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    diff = g.view(np.uint32) != w.view(np.uint32)
    zero = diff & (g == 0) & (w == 0)
    ulp = np.abs(g.astype(np.float64) - w.astype(np.float64)) / np.maximum(np.spacing(np.maximum(np.abs(g), np.abs(w))).astype(np.float64), 1e-45)
    print("%s: %d of %d elements differ in bits, %d of them in the sign of a zero only; largest difference %.2f ulp" % (what, diff.sum(), g.size, zero.sum(), ulp.max()))


def _args(c):
    return types.SimpleNamespace(**c._asdict())


def _offset(torch, a, off, dev="cuda"):
    """`a` on the device at `off` elements past a 256-byte aligned base: off 0 takes the 16-byte path, 1 the 4-byte one."""
    a = np.ascontiguousarray(a)
    buf = torch.empty(a.size + 8, dtype=torch.from_numpy(a).dtype, device=dev)
    v = buf[off:off + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == (off * a.itemsize) % 16
    return v


class _PA(object):
    """The tensors of the reference's PopArt(H, 1) on the device, weight and bias as Parameters (popart.py:30-41)."""

    def __init__(self, torch, st, off=0):
        self.beta, self.epsilon, self.norm_axes, self.output_shape = PL.BETA, PL.EPSILON, 1, 1
        for k in PL.STATE:
            t = _offset(torch, np.asarray(st[k], np.float32), off)
            setattr(self, k, torch.nn.Parameter(t) if k in ("weight", "bias") else t)

    def state(self):
        return {k: getattr(self, k).detach().cpu().numpy().copy() for k in PL.STATE}

    def load(self, torch, st):
        with torch.no_grad():
            for k in PL.STATE:
                getattr(self, k).copy_(torch.tensor(np.asarray(st[k], np.float32)))

    def debiased_mean_var(self):                                            # popart.py:85-89, for engine.denorm_scalars
        m = self.mean / self.debiasing_term.clamp(min=self.epsilon)
        return m, (self.mean_sq / self.debiasing_term.clamp(min=self.epsilon) - m ** 2).clamp(min=1e-2)


def _device(torch, inp, c, pa, off=0, install="replace", workspace=None):
    lg = _offset(torch, inp["logits"], off).requires_grad_(True)
    ft = _offset(torch, inp["features"], off).requires_grad_(True)
    f = {k: _offset(torch, inp[k], 0) for k in P.COLS + ("actions",)}
    if inp.get("available_actions") is not None:
        f["available_actions"] = _offset(torch, inp["available_actions"], off)
    w_obj, b_obj, s_obj = pa.weight, pa.bias, pa.stddev
    res = gmpe.ppo_losses_popart(lg, ft, f, _args(c), pa, install=install, workspace=workspace)
    got = {k: getattr(res, k).detach().cpu().numpy() for k in res._fields}
    res.actor_loss.backward()
    res.value_loss.backward()
    got.update(grad_logits=lg.grad.cpu().numpy(), grad_features=ft.grad.cpu().numpy(), grad_weight=w_obj.grad.cpu().numpy(),
               grad_bias=b_obj.grad.cpu().numpy(), state=pa.state(), same_objects=(pa.weight is w_obj, pa.bias is b_obj, pa.stddev is s_obj))
    return got


def _check(torch, got, inp, c, st_in, what="", stat_steps=1, stat_ref=None):
    """The device's `got` for `inp` from the PopArt arrays `st_in` against the float64 restatement (the module docstring's cut)."""
    B, H = inp["features"].shape
    free = PL.restate(inp, c, st_in, torch.float64)
    verr = np.abs(got["values"].astype(np.float64) - free["values"]) / PL.value_bound(free)
    print("%s values: %.3f of the dot-product bound" % (what, float(verr.max())))
    assert verr.max() <= 1.0, (what, "values", float(verr.max()))
    ref = PL.restate(inp, c, st_in, torch.float64, values=got["values"])
    Dp, Dv = ref["denom_policy"], ref["denom_value"]
    for k, scale, cc in (("action_log_probs", 1.0, P.C_DEV), ("imp_weights", 1.0, P.C_DEV), ("grad_logits", Dp, P.C_DEV), ("grad_features", Dv, PL.C_ROW)):
        e = float(P.row_err(got[k] * scale, ref[k] * scale).max())
        print("%s %s: %.1f units (bound %.0f)" % (what, k, e, cc))
        assert e <= cc, (what, k, e)
    F = np.abs(inp["features"].astype(np.float64))
    gw_tol = P.C_DEV * P.U * (F.sum(0, keepdims=True) + Dv * ref["abs_grad_weight"]) / Dv + P.U * np.abs(ref["grad_weight"])
    gb_tol = P.C_DEV * P.U * (B + Dv * ref["abs_grad_bias"]) / Dv + P.U * np.abs(ref["grad_bias"])
    assert (np.abs(got["grad_weight"] - ref["grad_weight"]) <= gw_tol).all(), (what, "grad_weight")
    assert (np.abs(got["grad_bias"] - ref["grad_bias"]) <= gb_tol).all(), (what, "grad_bias")
    b = P.scalar_bounds(ref, P.C_DEV)
    for k, bound in b.items():
        assert abs(float(got[k]) - float(ref[k])) <= bound + P.U * abs(float(ref[k])), (what, k)
    act = float(ref["policy_loss"]) - c.entropy_coef * float(ref["dist_entropy"])
    assert abs(float(got["actor_loss"]) - act) <= b["policy_loss"] + c.entropy_coef * b["dist_entropy"] + P.U * abs(act), what
    sref = stat_ref or ref["state"]
    for k in ("mean", "mean_sq", "debiasing_term"):
        assert abs(float(got["state"][k].reshape(-1)[0]) - float(sref[k].reshape(-1)[0])) <= stat_steps * PL.stat_tol(inp, k), (what, k)
    s64, w64, b64 = PL.rescale_layer(st_in["weight"], st_in["bias"], st_in["stddev"], got["state"]["mean"], got["state"]["mean_sq"])
    wb, bb = PL.layer_bounds(st_in["weight"], st_in["bias"], st_in["stddev"], got["state"]["mean"], s64)
    assert abs(float(got["state"]["stddev"][0]) - float(s64[0])) <= PL.C_LAYER * P.U * (1 + float(s64[0])), (what, "stddev")
    assert (np.abs(got["state"]["weight"] - w64) <= wb).all(), (what, "weight")
    assert (np.abs(got["state"]["bias"] - b64) <= bb).all(), (what, "bias")
    return ref


# ---------------------------------------------------------------------------------------------- 1
def test_exact_minibatches_are_the_bits_of_the_reference_run():
    import torch
    c, K, H, st, steps = fixture_case(np.load(GOLD), "exact")
    pa = _PA(torch, st)
    for i, (inp, out, st_after) in enumerate(steps):
        B = len(inp["returns"])
        old = (pa.weight, pa.bias, pa.stddev)
        got = _device(torch, inp, c, pa)
        for k in PL.STATE:                                                  # never depend on the values: the reference's bits in every minibatch
            assert np.array_equal(bits(got["state"][k]), bits(st_after[k])), (i, k)
        assert got["same_objects"] == (False, False, False)                # install="replace": new Parameters, the old objects hold the gradients
        assert isinstance(pa.weight, torch.nn.Parameter) and old[0].grad is not None and old[1].grad is not None and pa.weight.grad is None
        assert np.array_equal(old[0].detach().cpu().numpy(), st["weight"]) and np.array_equal(old[2].detach().cpu().numpy(), st["stddev"])
        if i == 0:                                                          # every dot product is exact in any order
            ref = PL.restate(inp, c, st, torch.float64, values=out["values"])
            _report("exact[0] values", got["values"], out["values"])
            _report("exact[0] grad_features", got["grad_features"], out["grad_features"])
            assert np.array_equal(bits(got["values"]), bits(out["values"]))
            assert np.array_equal(bits(got["grad_features"]), bits(out["grad_features"]))
        else:                                                               # rescaled weights: the sum's order shows in the last bits of the values
            ref = _check(torch, got, inp, c, st, "exact[%d]" % i)
            r32 = PL.restate(inp, c, st, torch.float32, values=got["values"])
            _report("exact[%d] grad_features vs float32 at the device's values" % i, got["grad_features"], r32["grad_features"])
            assert np.array_equal(bits(got["grad_features"]), bits(r32["grad_features"]))
        for k, terms, want in (("grad_weight", ref["abs_grad_weight"], out["grad_weight"] if i == 0 else ref["grad_weight"]),
                               ("grad_bias", ref["abs_grad_bias"], out["grad_bias"] if i == 0 else ref["grad_bias"])):
            tol = PL.sum_bound(B, terms) + P.U * np.abs(ref[k])
            assert (np.abs(got[k].astype(np.float64).reshape(ref[k].shape) - np.asarray(want, np.float64).reshape(ref[k].shape)) <= tol).all(), (i, k)
        if i == 0:
            assert abs(float(got["value_loss"]) - float(out["value_loss"])) <= PL.sum_bound(B, ref["abs_value"]) / ref["denom_value"]
            b = P.scalar_bounds(ref, P.C_DEV)
            for k in ("policy_loss", "dist_entropy", "ratio_mean"):         # exp and log enter these: the existing bound
                assert abs(float(got[k]) - float(out[k])) <= b[k], (i, k)
        st = st_after


# ---------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("name", ["g8", "g64"])
def test_generic_minibatches_through_the_device_path(name):
    import torch
    c, K, H, st, steps = fixture_case(np.load(GOLD), name)
    pa = _PA(torch, st)
    for i, (inp, out, st_after) in enumerate(steps):
        st_in = pa.state()                                                  # the device's own tensors before the call
        got = _device(torch, inp, c, pa)
        ref = _check(torch, got, inp, c, st_in, "%s[%d]" % (name, i))
        vb = PL.value_bound(ref)
        for k in ("mean", "mean_sq", "debiasing_term"):                     # and the reference's run: the noise of i + 1 batch means
            assert abs(float(got["state"][k].reshape(-1)[0]) - float(st_after[k].reshape(-1)[0])) <= (i + 1) * PL.stat_tol(inp, k), (i, k)
        if i == 0:                                                          # same layer on both sides: the run's values lie within two dot-product bounds
            assert (np.abs(got["values"].astype(np.float64) - out["values"]) <= 2 * vb).all()


# ---------------------------------------------------------------------------------------------- 3
def _case(B, K, H, kw, masks, seed=0):
    key = (B, K, H, tuple(sorted(kw.items())), masks, seed)
    if key not in _REF:
        c = PL.cfg(**kw)
        st = PL.fresh_popart(H, seed)
        _REF[key] = (PL.family(B, K, H, st, c, seed=seed, masks=masks), c, st)
    return _REF[key]


@pytest.mark.parametrize("H", PL.SHAPE_H)
@pytest.mark.parametrize("B", PL.SHAPE_ROWS)
def test_shapes(B, H):
    import torch
    kw = dict(huber_delta=0.5) if H % 2 else dict(clipped=(B % 2 == 1))
    inp, c, st = _case(B, 5, H, kw, "mixed" if B > 2 else "ones")
    _check(torch, _device(torch, inp, c, _PA(torch, st)), inp, c, st, "%dx%d" % (B, H))


@pytest.mark.parametrize("B,H,off", [(257, 64, 1), (300, 1024, 0), (65, 1024, 1)])
def test_the_four_byte_path_and_the_largest_hidden(B, H, off):
    import torch
    inp, c, st = _case(B, 5, H, dict(), "mixed")
    _check(torch, _device(torch, inp, c, _PA(torch, st, off), off), inp, c, st, "%dx%d+%d" % (B, H, off))


@pytest.mark.parametrize("case", PL.CASES, ids=lambda c: "%dx%dx%d" % c[:3])
def test_families_match_the_float64_restatement(case):
    import torch
    inp, c, st = _case(*case)
    _check(torch, _device(torch, inp, c, _PA(torch, st)), inp, c, st, "%dx%dx%d" % case[:3])


# ---------------------------------------------------------------------------------------------- 4
def test_in_place_install_keeps_the_parameters_and_gives_the_same_bits():
    import torch
    inp, c, st = _case(257, 9, 65, dict(huber_delta=0.5), "ones")
    a, pb = _device(torch, inp, c, _PA(torch, st)), _PA(torch, st)
    objs = (pb.weight, pb.bias, pb.stddev)
    b = _device(torch, inp, c, pb, install="in_place")
    assert a["same_objects"] == (False, False, False) and b["same_objects"] == (True, True, True)
    for k in a:
        if k == "state":
            for n in PL.STATE:
                assert np.array_equal(bits(a[k][n]), bits(b[k][n])), n
        elif k != "same_objects":
            assert np.array_equal(bits(a[k]), bits(b[k])), k
    assert objs[0].grad is not None and np.array_equal(bits(objs[0].grad.cpu().numpy()), bits(b["grad_weight"]))        # the gradients are on them
    assert objs[1].grad is not None and np.array_equal(bits(objs[1].grad.cpu().numpy()), bits(b["grad_bias"]))
    assert not np.array_equal(b["state"]["weight"], st["weight"])                                                        # and the storage was rewritten
    st2 = b["state"]
    inp2 = PL.family(257, 9, 65, st2, c, seed=1, masks="ones")
    objs[0].grad = objs[1].grad = None
    got = _device(torch, inp2, c, pb, install="in_place")                   # a second call reads the rewritten weights
    _check(torch, got, inp2, c, st2, "in_place second call")
    assert got["same_objects"] == (True, True, True)


# ---------------------------------------------------------------------------------------------- 5
def test_determinism_across_calls_and_alignments():
    import torch
    for case in ((257, 9, 65, dict(huber_delta=0.5), "ones"), (96, 5, 64, dict(pm=False, vm=False, clipped=False, huber=False), "mixed")):
        inp, c, st = _case(*case)
        runs = [_device(torch, inp, c, _PA(torch, st, off), off) for off in (0, 0, 1, 3)]
        for r in runs[1:]:
            for k, v in runs[0].items():
                if k == "state":
                    for n in PL.STATE:
                        assert np.array_equal(bits(v[n]), bits(r[k][n])), n
                elif k != "same_objects":
                    assert np.array_equal(bits(v), bits(r[k])), k


def test_graph_capture_moves_the_layer_as_eager_calls_do():
    """One call (install="in_place", a caller's workspace) with both backwards captured into a graph: replay r gives the bits of eager call r, and the six
    PopArt tensors after two replays are those after two eager calls."""
    import torch
    inp, c, st = _case(257, 9, 65, dict(huber_delta=0.5), "ones")
    pa = _PA(torch, st)
    lg = torch.tensor(inp["logits"], device="cuda", requires_grad=True)
    ft = torch.tensor(inp["features"], device="cuda", requires_grad=True)
    f = {k: torch.tensor(inp[k], device="cuda") for k in P.COLS + ("actions", "available_actions")}
    ws = torch.empty(gmpe.ppo_loss.popart_workspace_bytes(257, 65), dtype=torch.uint8, device="cuda")

    def call():
        res = gmpe.ppo_losses_popart(lg, ft, f, _args(c), pa, install="in_place", workspace=ws)
        gl, = torch.autograd.grad(res.actor_loss, lg)
        gf, gw, gb = torch.autograd.grad(res.value_loss, (ft, pa.weight, pa.bias))
        return tuple(getattr(res, k).detach() for k in res._fields) + (gl, gf, gw, gb)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()                                                              # warm-up on a side stream, as torch.cuda.graph wants
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    reps = 2
    pa.load(torch, st)
    eager, states = [], []
    for _ in range(reps):
        eager.append([t.cpu().numpy().copy() for t in call()])
        states.append(pa.state())
    assert all(not np.array_equal(states[0][k], states[1][k]) for k in PL.STATE)         # every call moves all six: two replays are told from one
    pa.load(torch, st)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = call()
    for t in static:
        t.fill_(-7.0)
    for r in range(reps):
        graph.replay()
        torch.cuda.synchronize()
        for i, (x, y) in enumerate(zip(eager[r], static)):
            assert np.array_equal(bits(x), bits(y.cpu().numpy())), "replay %d output %d" % (r, i)
    for k, v in pa.state().items():
        assert np.array_equal(bits(v), bits(states[-1][k])), k


# ---------------------------------------------------------------------------------------------- 6
def test_autograd_through_a_small_critic_body_matches_torch_ops():
    import torch
    inp, c, st = _case(300, 5, 32, dict(huber_delta=0.5), "ones")
    feats = torch.randn(300, 16, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    f = {k: torch.tensor(inp[k], device="cuda") for k in P.COLS + ("actions", "available_actions")}
    lg = torch.tensor(inp["logits"], device="cuda")
    t = lambda a: torch.tensor(np.asarray(a, np.float32), device="cuda")
    grads = {}
    for path, scale in (("fused", 1.0), ("torch", 1.0), ("fused", 1024.0)):
        torch.manual_seed(1)
        body = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.Tanh()).cuda()
        pa = _PA(torch, st)
        W, b = pa.weight, pa.bias
        h = body(feats)
        if path == "fused":
            value = gmpe.ppo_losses_popart(lg, h, f, _args(c), pa).value_loss
        else:                                                               # F.linear with the pre-update weights, then the restated loss as device torch ops
            v = torch.nn.functional.linear(h, W, b)
            r64 = PL.restate(dict(inp, features=h.detach().cpu().numpy()), c, st, torch.float64)
            mean, msq, db = (t(r64["state"][k]) for k in ("mean", "mean_sq", "debiasing_term"))
            dcl = db.clamp(min=PL.EPSILON)
            R = (f["returns"] - mean / dcl) / torch.sqrt((msq / dcl - (mean / dcl) ** 2).clamp(min=1e-2))
            vp, am = f["value_preds"], f["active_masks"]
            vpc = vp + (v - vp).clamp(-c.clip_param, c.clip_param)
            hub = lambda e, d: (abs(e) <= d).float() * e ** 2 / 2 + (e > d).float() * d * (abs(e) - d / 2)
            L = torch.max(hub(R - v, c.huber_delta), hub(R - vpc, c.huber_delta))
            value = (L * am).sum() / am.sum()
        (value * 0.5 * scale).backward()                                    # value_loss * value_loss_coef, as ppo_update
        grads[path, scale] = [p.grad.clone() for p in list(body.parameters()) + [W, b]]
    for a, b_ in zip(grads["fused", 1.0], grads["torch", 1.0]):
        assert torch.allclose(a, b_, rtol=P.C_DEV * P.U, atol=P.C_DEV * P.U), float((a - b_).abs().max())
    for a, b_ in zip(grads["fused", 1.0], grads["fused", 1024.0]):         # a non-unit incoming scalar, as a GradScaler sends: a power of two scales exactly
        assert torch.equal(a * 1024.0, b_)


def test_half_features_are_widened():
    import torch
    inp, c, st = _case(96, 5, 64, dict(pm=False, vm=False, clipped=False, huber=False), "mixed")
    f = {k: torch.tensor(inp[k], device="cuda") for k in P.COLS + ("actions",)}
    lg = torch.tensor(inp["logits"], device="cuda")
    half = torch.tensor(inp["features"], device="cuda").to(torch.bfloat16).requires_grad_(True)
    wide = half.detach().float().requires_grad_(True)
    a, b = gmpe.ppo_losses_popart(lg, half, f, _args(c), _PA(torch, st)), gmpe.ppo_losses_popart(lg, wide, f, _args(c), _PA(torch, st))
    assert torch.equal(a.value_loss, b.value_loss) and torch.equal(a.values, b.values) and a.value_loss.dtype == torch.float32
    a.value_loss.backward()
    b.value_loss.backward()
    assert half.grad.dtype == torch.bfloat16 and torch.equal(half.grad, wide.grad.to(torch.bfloat16))


# ---------------------------------------------------------------------------------------------- 7
def test_generator_sample_goes_in_as_it_comes_out():
    import torch
    from gmpe.engine import GmpeEngine
    from gmpe.rollout import DeviceRolloutBuffer
    T, N, A, H = 4, 6, 3, 64
    eng = GmpeEngine(gmpe.make_config(num_envs=N, num_agents=A, episode_length=T, seed=5), device=0)
    args = types.SimpleNamespace(gamma=0.99, gae_lambda=0.95, use_gae=True, use_proper_time_limits=False, use_valuenorm=False, use_popart=True,
                                 clip_param=0.2, huber_delta=10.0, entropy_coef=0.01)
    st = PL.fresh_popart(H, 3)
    st.update(mean=np.array([0.02], np.float32), mean_sq=np.array([0.3], np.float32), debiasing_term=np.array(0.05, np.float32),
              stddev=np.array([0.5], np.float32))                           # a layer that has seen data: denormalisation is no identity
    pa = _PA(torch, st)
    buf = DeviceRolloutBuffer(eng, T, args=args, policy_fields="all", learner_fields="all")
    buf.warmup()
    dev = eng.device
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    for t in range(T):
        act = torch.randint(0, 25, (N * A, 1), generator=g, device=dev)
        buf.insert_step(act.view(N, A).to(torch.int32), values=torch.randn((N * A, 1), generator=g, device=dev), actions=act,
                        action_log_probs=-3.2 + 0.1 * torch.randn((N * A, 1), generator=g, device=dev),
                        rnn_states=torch.zeros((N * A, 1, 64), device=dev), rnn_states_critic=torch.zeros((N * A, 1, 64), device=dev))
    buf.compute_returns(torch.zeros(N, A, 1), value_normalizer=pa)
    adv = buf.normalized_advantages(value_normalizer=pa).clone()
    n = 0
    c = PL.cfg(clip_param=0.2)
    for sample in buf.feed_forward_generator(adv, num_mini_batch=2):
        rows = sample[8].shape[0]
        lg = (0.3 * torch.randn((rows, 25), generator=g, device=dev)).requires_grad_(True)
        ft = torch.randn((rows, H), generator=g, device=dev).requires_grad_(True)
        st_in, w_obj, b_obj = pa.state(), pa.weight, pa.bias
        res = gmpe.ppo_losses_popart(lg, ft, sample, args, pa)
        res.actor_loss.backward()
        res.value_loss.backward()
        inp = dict(logits=lg.detach().cpu().numpy(), features=ft.detach().cpu().numpy(), actions=sample[8].cpu().numpy(),
                   available_actions=None if sample[15] is None else sample[15].cpu().numpy(), value_preds=sample[9].cpu().numpy(),
                   returns=sample[10].cpu().numpy(), active_masks=sample[12].cpu().numpy(), old_action_log_probs=sample[13].cpu().numpy(),
                   adv_targ=sample[14].cpu().numpy())
        got = {k: getattr(res, k).detach().cpu().numpy() for k in res._fields}
        got.update(grad_logits=lg.grad.cpu().numpy(), grad_features=ft.grad.cpu().numpy(), grad_weight=w_obj.grad.cpu().numpy(),
                   grad_bias=b_obj.grad.cpu().numpy(), state=pa.state())
        _check(torch, got, inp, c, st_in, "generator")
        n += 1
    assert n == 2
    eng.check_errors()
    eng.close()
