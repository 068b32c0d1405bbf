"""Returns, advantages and stop-action rows on the device (include/gmpe.h gmpe_compute_returns, gmpe_available_actions_from_dones) against the
reference's own vectors (tests/golden/returns_advantages.npz, available_actions.npz, made by tests/golden/make_returns_fixture.py) and against the
float32 NumPy restatement (tests/returns_lib.py, pinned to the reference by tests/test_returns_host.py) at the bench shapes and odd lane counts;
determinism, stream order after a collect, hipGraph replay, and the stop-action slots of a real July closed loop and of the open-loop collect."""
import os

import numpy as np
import pytest

import gmpe
import returns_lib as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
KEYS = [("gae" if g else "mc", "proper" if p else "plain", n) for g in (True, False) for p in (False, True) for n in ("none", "valuenorm", "popart")]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class _Norm(object):
    """Duck-typed ValueNorm / PopArt holding the statistics the reference's normaliser returned (on the host, as in the fixture's run)."""

    def __init__(self, mean, var, popart=False):
        import torch
        f = lambda: (torch.as_tensor(mean).reshape(1), torch.as_tensor(var).reshape(1))
        setattr(self, "debiased_mean_var" if popart else "running_mean_var", f)


def _run(torch, d, gae, proper, norm, normalized=True):
    dev = "cuda"
    g = lambda k: torch.as_tensor(d[k], device=dev).contiguous()
    vp, ret = g("value_preds"), g("returns_in")
    T = vp.shape[0] - 1
    adv = torch.empty_like(g("rewards"))
    advn = torch.empty_like(adv) if normalized else None
    gmpe.engine.compute_returns(g("rewards"), g("masks"), vp, ret, g("next_value"), gamma=float(d["gamma"]), gae_lambda=float(d["gae_lambda"]),
                                use_gae=gae, use_proper_time_limits=proper, bad_masks=g("bad_masks"), denorm=norm, advantages=adv,
                                active_masks=g("active_masks") if normalized else None, normalized=advn)
    torch.cuda.synchronize()
    assert adv.shape[0] == T
    return ret.cpu().numpy(), vp.cpu().numpy(), adv.cpu().numpy(), None if advn is None else advn.cpu().numpy()


@pytest.mark.parametrize("key", KEYS, ids=["_".join(k) for k in KEYS])
def test_returns_and_advantages_match_reference_fixture(key):
    import torch
    d = np.load(os.path.join(GOLD, "returns_advantages.npz"))
    kind, pr, name = key
    k = "_".join(key)
    # the reference's own (mean, sqrt(var)) pair: a host torch.sqrt elsewhere may round differently from the run that made the fixture
    norm = None if name == "none" else tuple(torch.as_tensor(d[name + s], device="cuda").reshape(1) for s in ("_mean", "_std"))
    ret, vp, adv, advn = _run(torch, d, kind == "gae", pr == "proper", norm)
    np.testing.assert_array_equal(_bits(ret), _bits(d["ret_" + k]))          # incl. the side effect returns[T] = next_value (MC branches)
    np.testing.assert_array_equal(_bits(vp), _bits(d["vp_" + k]))            # value_preds[T] = next_value (GAE branches), rest untouched
    np.testing.assert_array_equal(_bits(adv), _bits(d["adv_" + k]))
    np.testing.assert_allclose(advn, d["advn_" + k], rtol=0, atol=1e-5)
    # train's path on the buffer as compute_returns left it: advantages only, normalised in place
    a2 = torch.empty(adv.shape, dtype=torch.float32, device="cuda")
    gmpe.engine.compute_returns(None, None, torch.as_tensor(vp, device="cuda"), torch.as_tensor(ret, device="cuda"), advantages_only=True, denorm=norm,
                                advantages=a2, normalized=a2, active_masks=torch.as_tensor(d["active_masks"], device="cuda"))
    np.testing.assert_array_equal(_bits(a2.cpu().numpy()), _bits(advn))


def test_denorm_scalars_take_the_statistics_of_either_normaliser():
    import torch
    d = np.load(os.path.join(GOLD, "returns_advantages.npz"))
    for name in ("valuenorm", "popart"):
        m, s = gmpe.engine.denorm_scalars(_Norm(d[name + "_mean"], d[name + "_var"], popart=name == "popart"), "cuda")
        assert m.device.type == "cuda" and m.shape == s.shape == (1,)
        np.testing.assert_array_equal(m.cpu().numpy(), d[name + "_mean"])
        np.testing.assert_array_equal(s.cpu().numpy(), torch.sqrt(torch.as_tensor(d[name + "_var"])).numpy())   # sqrt where the statistics live
    with pytest.raises(TypeError):
        gmpe.engine.denorm_scalars(object(), "cuda")


def _random_inputs(rng, T, lanes):
    f32 = np.float32
    return dict(rewards=rng.randn(T, lanes, 1).astype(f32), value_preds=rng.randn(T + 1, lanes, 1).astype(f32),
                masks=(rng.rand(T + 1, lanes, 1) > 0.1).astype(f32), bad_masks=(rng.rand(T + 1, lanes, 1) > 0.05).astype(f32),
                active_masks=(rng.rand(T + 1, lanes, 1) > 0.2).astype(f32), returns_in=rng.randn(T + 1, lanes, 1).astype(f32),
                next_value=rng.randn(lanes, 1).astype(f32), gamma=0.99, gae_lambda=0.95)


SHAPES = [(25, 4096 * 10, "c3"), (25, 8192 * 32, "c4"), (25, 1, "1"), (25, 63, "63"), (7, 65, "65"), (25, 40961, "40961"), (1, 65, "T1")]


@pytest.mark.parametrize("T, lanes, tag", SHAPES, ids=[s[2] for s in SHAPES])
def test_random_inputs_match_numpy_restatement(T, lanes, tag):
    import torch
    rng = np.random.RandomState(lanes + T)
    d = _random_inputs(rng, T, lanes)
    mean, std = np.float32(0.37), np.float32(1.9)
    combos = [(g, p, n) for g in (True, False) for p in (False, True) for n in (False, True)]
    if tag == "c4":
        combos = [(True, False, False), (False, True, True)]
    for gae, proper, n in combos:
        norm = (torch.tensor([mean], device="cuda"), torch.tensor([std], device="cuda")) if n else None
        ret, vp, adv, advn = _run(torch, d, gae, proper, norm)
        den = (mean, std) if n else None
        eret, evp = R.np_returns(d["rewards"], d["masks"], d["value_preds"], d["returns_in"], d["next_value"], 0.99, 0.95, gae, proper, d["bad_masks"], den)
        eadv = R.np_advantages(eret, evp, den)
        label = "%s gae=%d proper=%d norm=%d" % (tag, gae, proper, n)
        np.testing.assert_array_equal(_bits(ret), _bits(eret), err_msg=label)
        np.testing.assert_array_equal(_bits(vp), _bits(evp), err_msg=label)
        np.testing.assert_array_equal(_bits(adv), _bits(eadv), err_msg=label)
        np.testing.assert_allclose(advn, R.np_normalized(eadv, d["active_masks"]), rtol=1e-5, atol=1e-5, err_msg=label)


def test_normalisation_edge_cases_and_determinism():
    import torch
    rng = np.random.RandomState(3)
    T, lanes = 6, 100
    d = _random_inputs(rng, T, lanes)
    d["active_masks"][:] = 0.0
    _, _, adv, advn = _run(torch, d, True, False, None)
    assert np.isnan(advn).all()                                                   # nothing active: np.nanmean of all-NaN
    d["active_masks"][3, 17] = 1.0                                                # one active entry: std 0, (adv - adv_k) / 1e-5
    _, _, adv, advn = _run(torch, d, True, False, None)
    assert advn[3, 17, 0] == 0.0
    np.testing.assert_allclose(advn, (adv - adv[3, 17, 0]) / np.float32(1e-5), rtol=1e-5)
    np.testing.assert_array_equal(_bits(advn), _bits((adv - adv[3, 17, 0]) / np.float32(1e-5)))   # mean = the entry, den = float32(1e-5): exact
    d = _random_inputs(np.random.RandomState(4), 25, 40960)
    a = _run(torch, d, True, True, None)
    b = _run(torch, d, True, True, None)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(_bits(x), _bits(y))                         # fixed-order merges: bitwise run to run


def test_graph_capture_replays_identically():
    import torch
    rng = np.random.RandomState(7)
    T, lanes = 25, 40960
    d = _random_inputs(rng, T, lanes)
    g = lambda k: torch.as_tensor(d[k], device="cuda").contiguous()
    ins = {k: g(k) for k in ("rewards", "masks", "bad_masks", "active_masks", "next_value")}
    vp, ret, adv = g("value_preds"), g("returns_in"), torch.zeros(T, lanes, 1, device="cuda")
    mean, std = torch.tensor([0.2], device="cuda"), torch.tensor([1.5], device="cuda")
    ws = torch.empty(gmpe.engine.returns_workspace_bytes(lanes), dtype=torch.uint8, device="cuda")

    def call():
        gmpe.engine.compute_returns(ins["rewards"], ins["masks"], vp, ret, ins["next_value"], gamma=0.99, gae_lambda=0.95, use_gae=True,
                                    use_proper_time_limits=True, bad_masks=ins["bad_masks"], denorm=(mean, std), advantages=adv,
                                    active_masks=ins["active_masks"], normalized=adv, workspace=ws)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()                                                                    # eager, on a side stream as torch.cuda.graph wants for warm-up
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    eager = [t.cpu().numpy().copy() for t in (ret, vp, adv)]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    ret[:T].zero_()
    adv.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(eager, (ret, vp, adv)):
        np.testing.assert_array_equal(_bits(x), _bits(y.cpu().numpy()))


def test_collect_then_compute_returns_on_one_stream_without_sync():
    import argparse
    import torch
    from gmpe.engine import GmpeEngine
    from gmpe.rollout import DeviceRolloutBuffer
    N, A, T = 512, 10, 25
    cfg = gmpe.make_config(num_envs=N, num_agents=A, episode_length=10, seed=5)      # every env ends its episode twice inside the rollout
    args = argparse.Namespace(gamma=0.99, gae_lambda=0.95, use_gae=True, use_proper_time_limits=False, use_valuenorm=True, use_popart=False)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        eng = GmpeEngine(cfg, device=0, adj_compact=True)
        buf = DeviceRolloutBuffer(eng, T, policy_fields="all", args=args)
        buf.warmup()
        rng = np.random.RandomState(1)
        acts = torch.as_tensor(rng.randint(0, cfg.n_actions, (T, N, A)).astype(np.int32), device="cuda")
        vals = torch.as_tensor(rng.randn(T, N, A, 1).astype(np.float32), device="cuda")
        buf.value_preds[:T].copy_(vals)
        nv = torch.as_tensor(rng.randn(N, A, 1).astype(np.float32), device="cuda")
        norm = _Norm(np.float32(0.5), np.float32(2.25))
        buf.collect(acts)                                                          # one rollout launch ...
        buf.compute_returns(nv, norm)                                              # ... then the returns, same stream, no sync
        ret = buf.returns.clone()
        buf.normalized_advantages(norm)
    s.synchronize()
    h = lambda t: t.cpu().numpy()
    den = (np.float32(0.5), np.float32(1.5))
    eret, evp = R.np_returns(h(buf.rewards), h(buf.masks), np.concatenate([h(vals), h(nv)[None]]), np.zeros((T + 1, N, A, 1), np.float32), h(nv),
                             0.99, 0.95, True, False, None, den)
    assert (h(buf.dones) != 0).any()
    np.testing.assert_array_equal(_bits(h(ret)), _bits(eret))
    np.testing.assert_allclose(h(buf.advantages), R.np_normalized(R.np_advantages(eret, evp, den), h(buf.active_masks)), rtol=1e-5, atol=1e-5)
    np.testing.assert_array_equal(h(buf.available_actions)[1:], R.np_available_actions(h(buf.dones), cfg.n_actions))
    eng.close()


def test_available_actions_match_reference_fixture():
    import torch
    d = np.load(os.path.join(GOLD, "available_actions.npz"))
    T, n = int(d["T"]), int(d["n_actions"])
    for ep in range(d["dones"].shape[0]):
        dones = torch.as_tensor(d["dones"][ep].astype(np.uint8), device="cuda")
        out = torch.full((T,) + tuple(dones.shape[1:]) + (n,), -1.0, device="cuda")
        gmpe.engine.available_actions_from_dones(dones, out)                        # the whole episode, one launch
        np.testing.assert_array_equal(out.cpu().numpy(), d["slots"][ep][1:])
        out.fill_(-1.0)
        for t in range(T):                                                          # the closed loop: one position per step
            gmpe.engine.available_actions_from_dones(dones, out, first=t, count=1)
            np.testing.assert_array_equal(out[t].cpu().numpy(), d["policy_avail"][ep][t])
        out.fill_(-1.0)
        gmpe.engine.available_actions_from_dones(dones, out, first=T - 2, count=T + 3)   # wraps: every position once
        np.testing.assert_array_equal(out.cpu().numpy(), d["slots"][ep][1:])


def _july_guided():
    import replay_lib
    path = os.path.join(GOLD, "july_A3_s2_guided.npz")
    d = np.load(path)
    return d, replay_lib.fixture_config(d, path, 1)


def _drive(torch, closed_loop, Tb):
    """The guided July fixture (agents finish, the env resets, the reference's positions are injected after each reset) through a
    DeviceRolloutBuffer with episode length Tb: insert_step per step (closed loop) or collect in segments that end at each reset / episode end."""
    from gmpe.engine import GmpeEngine
    from gmpe.rollout import DeviceRolloutBuffer
    d, cfg = _july_guided()
    eng = GmpeEngine(cfg, device=0)
    buf = DeviceRolloutBuffer(eng, Tb, policy_fields=("available_actions",))
    eng.set("prev_phase", d["init_prev_phase"][None])
    eng.set_tape(d["tape"][None])
    n_inj = [0]

    def inject():
        inj = d["inject"][n_inj[0]]; n_inj[0] += 1
        eng.set("x", inj[None, :, 0]); eng.set("y", inj[None, :, 1]); eng.set("s2", inj[None, :, 2]); eng.set("s3", inj[None, :, 3])
    buf.warmup()
    inject()
    act = d["act"].astype(np.int32)
    S = act.shape[0]
    episodes, dones, t = [], [], 0
    while t < S:
        if closed_loop:
            pos = buf.step
            rows = buf.available_actions_for(pos).cpu().numpy()
            exp = R.np_available_actions(buf.dones.cpu().numpy(), cfg.n_actions)[pos]   # the rule on the dones the engine emitted
            np.testing.assert_array_equal(rows, exp, err_msg="step %d" % t)
            buf.insert_step(torch.as_tensor(act[t][None], device="cuda"))
            K = 1
        else:
            K = 1
            while t + K < S and not d["did_reset"][t + K - 1] and buf.step + K < Tb:
                K += 1
            buf.collect(torch.as_tensor(act[t:t + K][:, None], device="cuda").contiguous(), num_steps=K)
        for k in range(K):
            if d["did_reset"][t + k]:
                inject()
        t += K
        if buf.step == 0:
            torch.cuda.synchronize()
            episodes.append(buf.available_actions.cpu().numpy().copy())
            dones.append(buf.dones.cpu().numpy().copy())
            buf.after_update()
    np.testing.assert_array_equal(np.array(dones).reshape(-1, 3)[:len(episodes) * Tb].astype(bool), d["done"][:len(episodes) * Tb])
    eng.close()
    return np.array(episodes), np.array(dones)


def test_available_actions_on_a_real_closed_loop_and_the_open_loop_collect():
    import torch
    Tb = 26
    closed, dones = _drive(torch, True, Tb)
    assert len(closed) == 5
    assert dones.all(-1).any() and (dones.any(-1) & ~dones.all(-1)).any()          # fully-done (reset) and partly-done env steps occur
    for ep in range(len(closed)):
        np.testing.assert_array_equal(closed[ep][1:], R.np_available_actions(dones[ep], closed.shape[-1]))
        if ep:
            np.testing.assert_array_equal(closed[ep][0], closed[ep - 1][Tb])       # after_update carries the last slot
    opened, dones_o = _drive(torch, False, Tb)
    np.testing.assert_array_equal(dones_o, dones)
    np.testing.assert_array_equal(opened, closed)
