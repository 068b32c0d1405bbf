"""The PPO loss arithmetic on the device (include/gmpe.h gmpe_ppo_loss, gmpe.ppo_losses) against the float64 restatement of the reference lines
(tests/ppo_loss_lib.py, pinned to the reference's own run by tests/test_ppo_loss_host.py) and against that run itself (tests/golden/ppo_loss.npz).

Bounds (ppo_loss_lib): per element C_DEV * U * (1 + |x|), gradients after multiplying back by the denominator; scalars (C_DEV + 2) * U * sum|term| /
denominator; ValueNorm state (log2(B) + 4) * U * mean|x|. C_DEV is four times the measured error of the reference's own float32 arithmetic.

On the ratio ties: a log-prob that is exact in float32 and float64 alike needs p[action] == 1 (a stop row, or K = 1), where [j == a] - p_j vanishes. The
rows with the ratio exactly at 1 - clip and 1 + clip are therefore the stop rows of the clip_param = 0 cases (ppo_loss_lib.RATIO_TIE_CASES: ratio == 1 == both
bounds); test_ratio_exactly_at_the_clip_bounds runs them. Their policy gradient is zero under either tie rule, so they cannot tell the rules apart: the inclusive
clamp rule is observable, and checked, on the value side (values - value_preds exactly at +-clip)."""
import os
import types

import numpy as np
import pytest

import gmpe
import ppo_loss_lib as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "ppo_loss.npz")
_REF = {}


def _args(c):
    return types.SimpleNamespace(**c._asdict())


class _VN(object):
    """The three tensors of the reference's ValueNorm(1, device=...) (valuenorm.py:34-39)."""

    def __init__(self, torch, state, dev="cuda"):
        self.norm_axes, self.per_element_update, self.beta, self.epsilon = 1, False, 0.99999, 1e-5
        for k, v in state.items():
            setattr(self, k, torch.tensor(np.asarray(v, np.float32), device=dev))

    def state(self):
        return {k: getattr(self, k).cpu().numpy() for k in ("running_mean", "running_mean_sq", "debiasing_term")}


def _offset(torch, a, off, dev="cuda"):
    """`a` on the device at `off` elements past a 256-byte aligned base: off 0 takes the 16-byte path, 1 the 4-byte one."""
    a = np.ascontiguousarray(a)
    buf = torch.empty(a.size + 8, dtype=torch.from_numpy(a).dtype, device=dev)
    v = buf[off:off + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == (off * a.itemsize) % 16
    return v


def _device(torch, inp, c, state=None, off=0, grad=True):
    lg = _offset(torch, inp["logits"], off).requires_grad_(grad)
    vl = _offset(torch, inp["values"], 0).requires_grad_(grad)
    f = {k: _offset(torch, inp[k], 0) for k in P.COLS + ("actions",)}
    if inp.get("available_actions") is not None:
        f["available_actions"] = _offset(torch, inp["available_actions"], off)
    vn = _VN(torch, state) if c.use_valuenorm else None
    res = gmpe.ppo_losses(lg, vl, f, _args(c), vn)
    got = {k: getattr(res, k).detach().cpu().numpy() for k in res._fields}
    if grad:
        res.actor_loss.backward()
        res.value_loss.backward()
        got["grad_logits"], got["grad_values"] = lg.grad.cpu().numpy(), vl.grad.cpu().numpy()
    got["state"] = vn.state() if vn else None
    return got


def _ref(case, seed=0):
    """The inputs of a case and their float64 restatement, computed once and shared."""
    key = (case[0], case[1], case[2], tuple(sorted(case[3].items())), case[4], case[5], seed)
    if key not in _REF:
        import torch
        inp, c, st = P.case_inputs(case, seed)
        _REF[key] = (inp, c, st, P.restate(inp, c, torch.float64, st))
    return _REF[key]


def _check(got, ref, inp, c, what=""):
    B = len(inp["logits"])
    nan = ref["denom_policy"] == 0 or ref["denom_value"] == 0
    for k, scale in (("action_log_probs", 1.0), ("imp_weights", 1.0), ("grad_logits", ref["denom_policy"]), ("grad_values", ref["denom_value"])):
        if scale == 0:
            continue
        e = float(P.row_err(got[k] * scale, ref[k] * scale).max())
        print("%s %s: %.1f units (bound %.0f)" % (what, k, e, P.C_DEV))
        assert e <= P.C_DEV, (what, k, e)
    b = P.scalar_bounds(ref, P.C_DEV) if not nan else {}
    for k, bound in b.items():
        err = abs(float(got[k]) - float(ref[k]))
        assert err <= bound + P.U * abs(float(ref[k])), (what, k, err, bound)            # + the rounding of the float64 scalar to float32
    if not nan:
        act = float(ref["policy_loss"]) - c.entropy_coef * float(ref["dist_entropy"])
        assert abs(float(got["actor_loss"]) - act) <= b["policy_loss"] + c.entropy_coef * b["dist_entropy"] + P.U * abs(act), what
    if c.use_valuenorm:
        for k, v in ref["state"].items():
            x = inp["returns"].astype(np.float64) ** 2 if k == "running_mean_sq" else inp["returns"].astype(np.float64)
            tol = (np.log2(B) + 4) * P.U * float(np.abs(x).mean()) if k != "debiasing_term" else 2 * P.U
            assert abs(float(got["state"][k].reshape(-1)[0]) - float(v.reshape(-1)[0])) <= tol, (what, k)


@pytest.mark.parametrize("case", P.ALL_CASES, ids=lambda c: "%s-%dx%d" % c[:3])
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset"])
def test_families_match_the_float64_restatement(case, off):
    import torch
    inp, c, st, ref = _ref(case)
    _check(_device(torch, inp, c, st, off), ref, inp, c, "%s-%dx%d" % case[:3])


SHAPE_B = [1, 3, 4, 63, 64, 65, 255, 256, 257, 1000, 4099]
SHAPE_K = [1, 2, 5, 8, 9, 24, 25, 33, 64]
# every B with a K and every K with a B (each B and K of the lists appears; odd / even K meet sizes below, at and above a wave, a tile and a workgroup)
SHAPES = sorted({(B, SHAPE_K[(3 * i) % len(SHAPE_K)]) for i, B in enumerate(SHAPE_B)} | {(SHAPE_B[(2 * i + 1) % len(SHAPE_B)], K) for i, K in enumerate(SHAPE_K)} |
                {(257, 64), (4099, 25), (1, 1), (65795, 2)})      # 65795 rows: 258 partials, more than one round of the merge's 256 threads


@pytest.mark.parametrize("B,K", SHAPES)
def test_shapes(B, K):
    import torch
    assert {b for b, _ in SHAPES} >= set(SHAPE_B) and {k for _, k in SHAPES} >= set(SHAPE_K)
    case = ("generic" if (B + K) % 2 else "edges", B, K, dict(valuenorm=B % 2 == 1), "mixed" if B > 2 else "ones", "given")
    inp, c, st, ref = _ref(case)
    for off in (0, 1):
        _check(_device(torch, inp, c, st, off), ref, inp, c, "%dx%d+%d" % (B, K, off))


@pytest.mark.parametrize("bits", range(16))
def test_all_flag_combinations(bits):
    import torch
    kw = dict(pm=bool(bits & 1), vm=bool(bits & 2), clipped=bool(bits & 4), huber=bool(bits & 8), huber_delta=0.5, valuenorm=bool(bits & 1) != bool(bits & 4))
    case = ("generic", 130, 9, kw, "mixed", "given")
    inp, c, st, ref = _ref(case)
    _check(_device(torch, inp, c, st), ref, inp, c, "flags%d" % bits)


@pytest.mark.parametrize("masks", ["ones", "mixed", "single", "zero"])
@pytest.mark.parametrize("avail", ["given", "none", "ones"])
def test_masks_and_availability(masks, avail):
    import torch
    case = ("edges", 131, 25, dict(), masks, avail)
    inp, c, st, ref = _ref(case)
    got = _device(torch, inp, c, st, grad=masks != "zero")
    if masks == "zero":                                              # 0 / 0 as the reference: NaN scalars, nothing waits to check
        for k in ("policy_loss", "dist_entropy", "actor_loss", "value_loss"):
            assert np.isnan(got[k]) and np.isnan(ref[k]), k
        assert abs(float(got["ratio_mean"]) - float(ref["ratio_mean"])) <= P.scalar_bounds(dict(ref, denom_policy=1.0, denom_value=1.0), P.C_DEV)["ratio_mean"] + P.U
        for k in ("action_log_probs", "imp_weights"):
            assert P.row_err(got[k], ref[k]).max() <= P.C_DEV
        return
    _check(got, ref, inp, c, "%s-%s" % (masks, avail))
    if avail == "given":
        one = inp["available_actions"].sum(1) == 1                   # stop rows: log-prob 0, a zero gradient row
        assert one.any() and (got["action_log_probs"][one] == 0).all() and (got["grad_logits"][one] == 0).all()
        assert (got["grad_logits"][inp["available_actions"] == 0] == 0).all()      # no gradient reaches a masked entry


def test_int64_actions_give_the_bits_of_float32_actions():
    import torch
    case = ("generic", 257, 25, dict(), "mixed", "given")
    inp, c, st, ref = _ref(case)
    a, b = _device(torch, inp, c, st), _device(torch, dict(inp, actions=inp["actions"].astype(np.int64)), c, st)
    for k in a:
        if k != "state":
            np.testing.assert_array_equal(a[k].view(np.uint32), b[k].view(np.uint32), err_msg=k)


def test_exact_tie_rows_follow_the_tie_rules():
    import torch
    case = ("ties", 256, 9, dict(huber=False), "mixed", "given")
    assert case in P.ALL_CASES
    inp, c, st, ref = _ref(case)
    got = _device(torch, inp, c, st)
    gaps = P.decision_gaps(ref["decisions"], c)
    D = ref["denom_value"]
    w = inp["active_masks"].reshape(-1).astype(np.float64)
    mirror = (gaps["branches"].reshape(-1) == 0) & (np.abs(ref["decisions"]["d"].reshape(-1)) > c.clip_param)
    assert mirror.sum() >= 32
    e_o = ref["decisions"]["e_o"].reshape(-1)
    mean_rule = w * 0.5 * (-e_o + 0.0)                               # the mean of the original branch's -e and the clipped branch's 0 (outside the clip)
    assert P.row_err(got["grad_values"].reshape(-1)[mirror] * D, mean_rule[mirror]).max() <= P.C_DEV
    assert (np.abs(mean_rule[mirror & (w > 0)]) > 0.1).all()         # and neither branch's own gradient would pass
    at = (gaps["d_hi"].reshape(-1) == 0) | (gaps["d_lo"].reshape(-1) == 0)      # values - value_preds exactly at +-clip: the clipped branch still passes gradient
    assert at.sum() >= 64
    assert P.row_err(got["grad_values"].reshape(-1)[at] * D, ref["grad_values"].reshape(-1)[at] * D).max() <= P.C_DEV
    tie = gaps["surr"].reshape(-1) == 0
    assert tie.any()
    assert P.row_err(got["grad_logits"][tie] * ref["denom_policy"], ref["grad_logits"][tie] * ref["denom_policy"]).max() <= P.C_DEV


@pytest.mark.parametrize("case", P.RATIO_TIE_CASES, ids=lambda c: "%s-%dx%d" % c[:3])
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset"])
def test_ratio_exactly_at_the_clip_bounds(case, off):
    import torch
    inp, c, st, ref = _ref(case)
    gaps = P.decision_gaps(ref["decisions"], c)
    at = (gaps["ratio_lo"].reshape(-1) == 0) & (gaps["ratio_hi"].reshape(-1) == 0)
    assert at.sum() >= 50
    got = _device(torch, inp, c, st, off)
    for k in got:
        assert k == "state" or np.isfinite(got[k]).all(), k
    assert (got["imp_weights"].reshape(-1)[at] == 1.0).all() and (got["action_log_probs"].reshape(-1)[at] == 0.0).all()
    assert (got["grad_logits"][at] == 0.0).all() and (ref["grad_logits"][at] == 0.0).all()       # the tie rule's value: adv * ratio * ([j == a] - p_j) = 0
    _check(got, ref, inp, c, "ratio-tie")                                                          # every row and the scalars within the bounds


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_reference_minibatches_through_the_device_path(name):
    import torch
    from test_ppo_loss_host import fixture_case
    c, K, steps = fixture_case(np.load(GOLD), name)
    vn = _VN(torch, P.fresh_state()) if c.use_valuenorm else None
    st64 = P.fresh_state() if c.use_valuenorm else None
    for i, (inp, out, st) in enumerate(steps):
        ref = P.restate(inp, c, torch.float64, st64)                 # for the denominators and the sums of |term| of the bounds
        lg = torch.tensor(inp["logits"], device="cuda", requires_grad=True)
        vl = torch.tensor(inp["values"], device="cuda", requires_grad=True)
        sample = (None,) * 8 + tuple(torch.tensor(inp[k], device="cuda") for k in ("actions", "value_preds", "returns")) + (None,) + \
            tuple(torch.tensor(inp[k], device="cuda") for k in ("active_masks", "old_action_log_probs", "adv_targ", "available_actions"))
        res = gmpe.ppo_losses(lg, vl, sample, _args(c), vn)          # the ValueNorm is carried across the three calls
        res.actor_loss.backward()
        res.value_loss.backward()
        got = dict(grad_logits=lg.grad.cpu().numpy(), grad_values=vl.grad.cpu().numpy(), action_log_probs=res.action_log_probs.cpu().numpy(),
                   imp_weights=res.imp_weights.cpu().numpy())
        for k, scale in (("action_log_probs", 1.0), ("imp_weights", 1.0), ("grad_logits", ref["denom_policy"]), ("grad_values", ref["denom_value"])):
            x = ref[k] * scale
            e = float((np.abs(got[k] * scale - out[k] * scale) / (P.U * (1 + np.abs(x)))).max())
            print("%s[%d] %s vs the reference's run: %.1f units (bound %.0f)" % (name, i, k, e, P.C_DEV))
            assert e <= P.C_DEV, (name, i, k, e)
        b = P.scalar_bounds(ref, P.C_DEV)
        for k in ("policy_loss", "dist_entropy", "value_loss", "ratio_mean"):
            assert abs(float(getattr(res, k).detach()) - float(out[k])) <= b[k], (name, i, k)
        if c.use_valuenorm:
            B = len(inp["returns"])
            for k, v in st.items():
                x = inp["returns"].astype(np.float64) ** 2 if k == "running_mean_sq" else inp["returns"].astype(np.float64)
                tol = (np.log2(B) + 4) * P.U * float(np.abs(x).mean())
                assert abs(float(getattr(vn, k).cpu().reshape(-1)[0]) - float(v.reshape(-1)[0])) <= tol, (name, i, k)
            st64 = ref["state"]


def test_determinism_across_calls_and_alignments():
    import torch
    case = ("generic", 1000, 33, dict(pm=False, vm=False), "mixed", "given")
    inp, c, st, _ = _ref(case)
    case2 = ("generic", 257, 25, dict(valuenorm=True), "mixed", "given")
    for inp, c, st in ((inp, c, st), _ref(case2)[:3]):
        runs = [_device(torch, inp, c, st, off) for off in (0, 0, 1, 3)]
        for r in runs[1:]:
            for k, v in runs[0].items():
                if k == "state":
                    assert v is None or all((v[n].view(np.uint32) == r[k][n].view(np.uint32)).all() for n in v)
                else:
                    np.testing.assert_array_equal(v.view(np.uint32), r[k].view(np.uint32), err_msg=k)


def test_graph_capture_replays_identically():
    """Forward and both backwards of one minibatch captured into a graph: every replay gives the bits of the eager call made in the same ValueNorm state,
    and the three state tensors after r replays are those after r eager calls."""
    import torch
    case = ("generic", 257, 25, dict(valuenorm=True), "mixed", "given")
    inp, c, st, _ = _ref(case)
    assert c.use_valuenorm
    lg = torch.tensor(inp["logits"], device="cuda", requires_grad=True)
    vl = torch.tensor(inp["values"], device="cuda", requires_grad=True)
    f = {k: torch.tensor(inp[k], device="cuda") for k in P.COLS + ("actions", "available_actions")}
    vn = _VN(torch, st)
    ws = torch.empty(gmpe.ppo_loss.workspace_bytes(257), dtype=torch.uint8, device="cuda")
    names = ("running_mean", "running_mean_sq", "debiasing_term")

    def reset():
        for k in names:
            getattr(vn, k).copy_(torch.tensor(np.asarray(st[k], np.float32)))

    def call():
        res = gmpe.ppo_losses(lg, vl, f, _args(c), vn, workspace=ws)
        gl, = torch.autograd.grad(res.actor_loss, lg)
        gv, = torch.autograd.grad(res.value_loss, vl)
        return tuple(getattr(res, k).detach() for k in res._fields) + (gl, gv)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()                                                       # warm-up on a side stream, as torch.cuda.graph wants
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    reps = 3
    reset()
    eager, states = [], []
    for _ in range(reps):
        eager.append([t.cpu().numpy().copy() for t in call()])
        states.append(vn.state())
    eager_state = states[-1]
    assert all((states[0][k] != eager_state[k]).all() for k in names)                # every call moves the state: r replays must be told from one
    reset()
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
            np.testing.assert_array_equal(x.view(np.uint32), y.cpu().numpy().view(np.uint32), err_msg="replay %d output %d" % (r, i))
    for k, v in vn.state().items():
        np.testing.assert_array_equal(v.view(np.uint32), eager_state[k].view(np.uint32), err_msg=k)


def _torch_ops(torch, logits, values, f, c):
    """The same arithmetic as device torch ops (float32, autograd), valuenorm off."""
    x = logits.clone()
    x[f["available_actions"] == 0] = P.FMIN32
    dist = torch.distributions.Categorical(logits=x)
    logp = dist.log_prob(f["actions"].squeeze(-1)).unsqueeze(-1)
    am = f["active_masks"]
    ent = (dist.entropy() * am.squeeze(-1)).sum() / am.sum()
    ratio = torch.exp(logp - f["old_action_log_probs"])
    s1, s2 = ratio * f["adv_targ"], torch.clamp(ratio, 1.0 - c.clip_param, 1.0 + c.clip_param) * f["adv_targ"]
    policy = (-torch.min(s1, s2) * am).sum() / am.sum()
    vp, R = f["value_preds"], f["returns"]
    vpc = vp + (values - vp).clamp(-c.clip_param, c.clip_param)

    def huber(e, d):
        return (abs(e) <= d).float() * e ** 2 / 2 + (e > d).float() * d * (abs(e) - d / 2)
    L = torch.max(huber(R - values, c.huber_delta), huber(R - vpc, c.huber_delta))
    return policy - ent * c.entropy_coef, (L * am).sum() / am.sum()


def test_autograd_through_a_small_head_matches_torch_ops():
    import torch
    case = ("generic", 300, 5, dict(huber_delta=0.5), "ones", "given")
    inp, c, st, _ = _ref(case)
    torch.manual_seed(0)
    feats = torch.randn(300, 16, device="cuda")
    f = {k: torch.tensor(inp[k], device="cuda") for k in P.COLS + ("actions", "available_actions")}
    grads = {}
    for path, scale in (("fused", 1.0), ("torch", 1.0), ("fused", 1024.0)):
        torch.manual_seed(1)
        body = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.Tanh()).cuda()
        head, vhead = torch.nn.Linear(32, 5).cuda(), torch.nn.Linear(32, 1).cuda()
        params = list(body.parameters()) + list(head.parameters()) + list(vhead.parameters())
        h = body(feats)
        logits, values = head(h), vhead(h)
        if path == "fused":
            res = gmpe.ppo_losses(logits, values, f, _args(c))
            actor, value = res.actor_loss, res.value_loss
        else:
            actor, value = _torch_ops(torch, logits, values, f, c)
        (actor * scale).backward(retain_graph=True)
        (value * 0.5 * scale).backward()                             # value_loss * value_loss_coef, as ppo_update
        grads[path, scale] = [p.grad.clone() for p in params]
    for a, b in zip(grads["fused", 1.0], grads["torch", 1.0]):
        assert torch.allclose(a, b, rtol=P.C_DEV * P.U, atol=P.C_DEV * P.U), float((a - b).abs().max())
    for a, b in zip(grads["fused", 1.0], grads["fused", 1024.0]):   # a non-unit incoming scalar, as a GradScaler sends: a power of two scales exactly
        assert torch.equal(a * 1024.0, b)
    only = []
    for scale in (1.0, 1024.0):                                      # the scalar alone: gradients scale exactly (a power of two)
        lg = torch.tensor(inp["logits"], device="cuda", requires_grad=True)
        vl = torch.tensor(inp["values"], device="cuda", requires_grad=True)
        res = gmpe.ppo_losses(lg, vl, f, _args(c))
        (res.actor_loss * scale).backward()
        (res.value_loss * scale).backward()
        only.append((lg.grad, vl.grad))
    assert torch.equal(only[0][0] * 1024.0, only[1][0]) and torch.equal(only[0][1] * 1024.0, only[1][1])


def test_half_logits_are_widened():
    import torch
    case = ("generic", 64, 64, dict(huber=False), "mixed", "none")
    inp, c, st, _ = _ref(case)
    half = torch.tensor(inp["logits"], device="cuda").to(torch.bfloat16).requires_grad_(True)
    wide = half.detach().float().requires_grad_(True)
    f = {k: torch.tensor(inp[k], device="cuda") for k in P.COLS + ("actions",)}
    vl = torch.tensor(inp["values"], device="cuda")
    a, b = gmpe.ppo_losses(half, vl, f, _args(c)), gmpe.ppo_losses(wide, vl, f, _args(c))
    assert torch.equal(a.actor_loss, b.actor_loss) and a.actor_loss.dtype == torch.float32
    a.actor_loss.backward()
    b.actor_loss.backward()
    assert half.grad.dtype == torch.bfloat16 and torch.equal(half.grad, wide.grad.to(torch.bfloat16))


def test_generator_sample_goes_in_as_it_comes_out():
    import torch
    from gmpe.engine import GmpeEngine
    from gmpe.rollout import DeviceRolloutBuffer
    T, N, A = 4, 6, 3
    eng = GmpeEngine(gmpe.make_config(num_envs=N, num_agents=A, episode_length=T, seed=5), device=0)
    args = types.SimpleNamespace(gamma=0.99, gae_lambda=0.95, use_gae=True, use_proper_time_limits=False, use_valuenorm=False, use_popart=False,
                                 clip_param=0.2, huber_delta=10.0, entropy_coef=0.01)
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
    buf.compute_returns(torch.zeros(N, A, 1))
    adv = buf.normalized_advantages().clone()
    n = 0
    for sample in buf.feed_forward_generator(adv, num_mini_batch=2):
        rows = sample[8].shape[0]
        lg = (0.3 * torch.randn((rows, 25), generator=g, device=dev)).requires_grad_(True)
        vl = torch.randn((rows, 1), generator=g, device=dev).requires_grad_(True)
        res = gmpe.ppo_losses(lg, vl, sample, args)
        res.actor_loss.backward()
        res.value_loss.backward()
        inp = dict(logits=lg.detach().cpu().numpy(), values=vl.detach().cpu().numpy(), actions=sample[8].cpu().numpy(),
                   available_actions=None if sample[15] is None else sample[15].cpu().numpy(), value_preds=sample[9].cpu().numpy(),
                   returns=sample[10].cpu().numpy(), active_masks=sample[12].cpu().numpy(), old_action_log_probs=sample[13].cpu().numpy(),
                   adv_targ=sample[14].cpu().numpy())
        c = P.cfg(clip_param=0.2)
        ref = P.restate(inp, c, torch.float64)
        got = {k: getattr(res, k).detach().cpu().numpy() for k in res._fields}
        got.update(grad_logits=lg.grad.cpu().numpy(), grad_values=vl.grad.cpu().numpy())
        # rollout data is what it is: rows whose decisions fall inside the margin are not excluded, the restatement must simply agree on them (it does
        # unless a comparison flips within rounding, which these smooth random inputs do not bring about)
        _check(got, ref, inp, c, "generator")
        n += 1
    assert n == 2
    eng.check_errors()
    eng.close()
