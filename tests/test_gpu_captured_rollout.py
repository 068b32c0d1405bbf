"""gmpe.policy.CapturedRollout — one episode's rollout captured as a graph and replayed — against the eager gmpe.policy.rollout on a twin engine with
the same networks, and run(..., captured=True) against run(..., install="in_place") on twin set-ups, bit for bit: a replay launches the same kernels
on the same inputs in the same order, and nothing on this path uses atomics, so equality is the expectation, not a tolerance. The set-up is
tests/test_gpu_collect.py's: N = 8 envs of A = 3 agents, T = 9 steps of envs whose time limit is 6, so dones fall inside every rollout (_compare
asserts that some rows are done and not all); one case has its own N = 5, T = 7, limit 4, whose 15 rows leave the last GNN tile of four graphs partly
filled, on engines made with GMPE_G=3, so that N is no multiple of the env tile either (by itself gmpe_create picks tiles of one env at this size).
A step captured directly with the engine's timing enabled covers gmpe_step's own question to its stream. The table-only buffer is
tests/test_gpu_policy_table.py's, run()'s twins are tests/test_gpu_infos.py's."""
import types

import numpy as np
import pytest
import torch

import gmpe
import gnn_lib as G
import test_gpu_infos as TI
import test_gpu_policy_table as TT
from gmpe import policy
from test_gpu_act_buffer import A, N, T, _same
from test_gpu_collect import CASES, STORED, _ValueNorm, _compare, _setup
from test_gpu_policy import DEV, K, _Net

pytestmark = pytest.mark.gpu
NORM_TENSORS = ("running_mean", "running_mean_sq", "debiasing_term", "weight", "bias", "stddev", "mean", "mean_sq")


def _same0(a, b, what):
    _same(a.reshape(-1), b.reshape(-1), what)               # a 0-dim tensor too


def _close(engines):
    for e in engines:
        e.check_errors()
        e.close()


def _same_states(ea, eb, what):
    sa, sb = ea.get_state(), eb.get_state()
    assert list(sa) == list(sb)
    for k in sa:
        assert sa[k].dtype == sb[k].dtype and sa[k].shape == sb[k].shape and sa[k].tobytes() == sb[k].tobytes(), "%s: engine state %s" % (what, k)


def _snapshot(buf, eng, actor, critic, vn):
    """everything a rollout could write and everything its graph holds by address, on the host: buffer arrays, counters, engine state and binding,
    parameters, normaliser tensors"""
    torch.cuda.synchronize()
    out = {"buffer." + k: t.cpu().numpy().copy() for k, t in buf._arrays() if k != "_act_draw_dev"}
    assert {"buffer.obs", "buffer.rewards", "buffer.returns", "buffer.rnn_states", "buffer.info", "buffer._act_idx"} <= set(out)
    out.update({"engine." + k: v for k, v in eng.get_state().items()})
    out.update({"actor." + k: p.detach().cpu().numpy().copy() for k, p in actor.named_parameters()})
    out.update({"critic." + k: p.detach().cpu().numpy().copy() for k, p in critic.named_parameters()})
    for tag, o in (("vn.", vn), ("v_out.", getattr(critic, "v_out", None))):
        if o is not None:
            out.update({tag + k: getattr(o, k).detach().cpu().numpy().copy() for k in NORM_TENSORS if isinstance(getattr(o, k, None), torch.Tensor)})
    out["act_draw"], out["step"] = np.int64(buf.act_draw), np.int64(buf.step)
    out["bound"] = np.array([0 if getattr(eng.out, k) is None else getattr(eng.out, k).data_ptr() for k in type(eng.out).__slots__], dtype=np.uint64)
    return out


def _unchanged(before, after, what):
    assert sorted(before) == sorted(after), (what, sorted(set(before) ^ set(after)))
    for k in before:
        assert np.asarray(before[k]).tobytes() == np.asarray(after[k]).tobytes(), "%s: %s changed" % (what, k)


# ------------------------------------------------------------------------------------------------ 1: replay against eager
@pytest.mark.parametrize("case", list(CASES))
def test_three_replays_are_three_eager_rollouts_bit_for_bit(case):
    kw = CASES[case]
    cfg, engines, (ba, bb), actor, critic, vn = _setup(**kw)
    cap = policy.CapturedRollout(actor, critic, bb, vn)
    for ep in range(3):
        want, got = policy.rollout(actor, critic, ba, vn), cap.replay()
        assert want is ba.returns and got is bb.returns
        _compare(ba, bb, "%s episode %d" % (case, ep))
        assert bb.act_draw == (ep + 1) * T
        out = engines[1].out                                # the engine's current outputs are slot T's, as after rollout
        assert out.obs.data_ptr() == bb.obs[T].data_ptr() and out.reward.data_ptr() == bb.rewards[T - 1].data_ptr()
        assert out.done.data_ptr() == bb.dones[T - 1].data_ptr() and out.adj.data_ptr() == bb._adj[T].data_ptr()
        for b in (ba, bb):
            b.after_update()
    _same_states(engines[0], engines[1], case)
    _close(engines)


# ------------------------------------------------------------------------------------------------ 2: construction changes nothing
@pytest.mark.parametrize("case", ["recurrent-valuenorm-cent", "recurrent-popart-own"])
def test_construction_leaves_everything_as_it_found_it(case):
    cfg, engines, (ba, bb), actor, critic, vn = _setup(**CASES[case])
    # from a buffer in use: one episode played and carried over, so every array holds something
    policy.rollout(actor, critic, bb, vn)
    bb.after_update()
    bb.act_draw_counter()
    before = _snapshot(bb, engines[1], actor, critic, vn)
    counter = bb._act_draw_dev.clone()
    cap = policy.CapturedRollout(actor, critic, bb, vn)
    after = _snapshot(bb, engines[1], actor, critic, vn)
    _unchanged(before, after, "construction")
    assert torch.equal(counter, bb._act_draw_dev) and cap.counter is bb._act_draw_dev
    assert bb.step == 0 and bb.act_draw == T
    # ... and the episode that follows is the eager one's
    policy.rollout(actor, critic, ba, vn)
    ba.after_update()
    policy.rollout(actor, critic, ba, vn)
    cap.replay()
    _compare(ba, bb, "the replay after construction")
    _close(engines)


# ------------------------------------------------------------------------------------------------ 3, 4: values are followed, addresses are guarded
def test_in_place_changes_are_followed_and_a_moved_tensor_raises():
    cfg, engines, (ba, bb), actor, critic, vn = _setup(**CASES["recurrent-valuenorm-cent"])
    cap = policy.CapturedRollout(actor, critic, bb, vn)
    opts = [torch.optim.Adam(net.parameters(), lr=1e-2) for net in (actor, critic)]
    g = torch.Generator(device=DEV).manual_seed(7)
    previous = None
    for ep in range(2):
        policy.rollout(actor, critic, ba, vn)
        cap.replay()
        _compare(ba, bb, "episode %d" % ep)
        if previous is not None:
            assert not torch.equal(previous[0], bb.value_preds) and not torch.equal(previous[1], bb.returns) and not torch.equal(previous[2], bb.actions)
        previous = (bb.value_preds.clone(), bb.returns.clone(), bb.actions.clone())
        for b in (ba, bb):
            b.after_update()
        # an optimiser step on both networks and a ValueNorm update, in place: the networks are shared, so the eager twin sees the same values
        ptrs = [p.data_ptr() for net in (actor, critic) for p in net.parameters()]
        for net, opt in zip((actor, critic), opts):
            for p in net.parameters():
                p.grad = torch.randn(p.shape, generator=g, device=DEV)
            opt.step()
        vn.running_mean.add_(0.25), vn.running_mean_sq.mul_(1.5), vn.debiasing_term.fill_(0.75)
        assert ptrs == [p.data_ptr() for net in (actor, critic) for p in net.parameters()]
    # 4: a parameter that moved
    name, moved = list(critic.named_parameters())[3]
    before = _snapshot(bb, engines[1], actor, critic, vn)
    moved.data = moved.data.clone()
    with pytest.raises(RuntimeError, match=r"CapturedRollout.replay: critic\.%s is not where it was captured" % name.replace(".", r"\.")):
        cap.replay()
    _unchanged(before, _snapshot(bb, engines[1], actor, critic, vn), "a refused replay")
    # ... a normaliser tensor and a buffer array likewise, each named
    critic_back = policy.CapturedRollout(actor, critic, bb, vn)
    vn.running_mean = vn.running_mean.clone()
    with pytest.raises(RuntimeError, match=r"value_normalizer\.running_mean is not where it was captured"):
        critic_back.replay()
    again = policy.CapturedRollout(actor, critic, bb, vn)
    bb.rewards = bb.rewards.clone()
    with pytest.raises(RuntimeError, match=r"buffer\.rewards is not where it was captured"):
        again.replay()
    # a graph built over the moved tensors replays, and is the eager rollout
    cap = policy.CapturedRollout(actor, critic, bb, vn)
    policy.rollout(actor, critic, ba, vn)
    cap.replay()
    _compare(ba, bb, "a new graph over the moved tensors")
    _close(engines)


# ------------------------------------------------------------------------------------------------ 5: eager and captured interleave
def test_eager_replay_eager_is_three_eager_episodes():
    cfg, engines, (ba, bb), actor, critic, vn = _setup(**CASES["recurrent-valuenorm-cent"])
    cap = policy.CapturedRollout(actor, critic, bb, vn)
    for ep, how in enumerate((policy.rollout, None, policy.rollout)):
        policy.rollout(actor, critic, ba, vn)
        if how is None:
            cap.replay()                                    # the counter is brought to act_draw first: T eager steps ran since construction
        else:
            how(actor, critic, bb, vn)
        _compare(ba, bb, "episode %d" % ep)
        assert bb.act_draw == (ep + 1) * T
        for b in (ba, bb):
            b.after_update()
    _same_states(engines[0], engines[1], "eager, replay, eager")
    _close(engines)


# ------------------------------------------------------------------------------------------------ 6: partial tiles
def test_fifteen_rows_and_five_envs_over_two_episodes(monkeypatch):
    from gmpe.engine import GmpeEngine
    from gmpe.rollout import DeviceRolloutBuffer
    n, a, t = 5, 3, 7
    cfg = gmpe.make_config(num_envs=n, num_agents=a, episode_length=4, seed=17)
    # by itself gmpe_create picks tiles of one env at this size: a tile of three (a performance knob: results must not change) leaves the last one partly filled
    monkeypatch.setenv("GMPE_G", "3"); monkeypatch.setenv("GMPE_BLOCK", "128")
    engines = [GmpeEngine(cfg, device=0) for _ in range(2)]
    key = G.ACTOR if int(cfg.node_feats) == 7 else G.ROTATE
    assert G.CONFIGS[key]["F"] == int(cfg.node_feats) and int(cfg.n_actions) == K
    tile = engines[0].tuning()["G"]
    assert tile > 1 and n % tile != 0                       # N is no multiple of the env tile: the last tile of three envs holds two
    assert (n * a) % 4 == 3                                 # the last GNN tile of four graphs holds three
    actor = _Net(key, engines[0].D, "act").to(DEV)
    critic = _Net(key, engines[0].D, "v_out", use_cent_obs=True, seed=12).to(DEV)
    vn = _ValueNorm(DEV)
    vn.running_mean.fill_(0.3), vn.running_mean_sq.fill_(0.7), vn.debiasing_term.fill_(0.5)
    args = types.SimpleNamespace(gamma=0.99, gae_lambda=0.95, use_gae=True, use_proper_time_limits=False, use_valuenorm=True, use_popart=False)
    ba, bb = [DeviceRolloutBuffer(e, t, use_centralized_V=False, policy_fields="all", learner_fields="all", args=args, recurrent_N=1, hidden_size=64)
              for e in engines]
    for b in (ba, bb):
        b.warmup()
    cap = policy.CapturedRollout(actor, critic, bb, vn)
    for ep in range(2):
        policy.rollout(actor, critic, ba, vn)
        cap.replay()
        torch.cuda.synchronize()
        dn = ba.dones.bool().cpu().numpy()
        assert dn.any() and not dn.all()
        for k in STORED:
            _same(getattr(ba, k), getattr(bb, k), "episode %d %s" % (ep, k))
        assert ba.step == bb.step == 0 and ba.act_draw == bb.act_draw == (ep + 1) * t
        for b in (ba, bb):
            b.after_update()
    _same_states(engines[0], engines[1], "5 x 3")
    _close(engines)


# ------------------------------------------------------------------------------------------------ 7: a table-only buffer
def test_a_table_only_buffer_replays_what_it_rolls_out():
    _, ea, ba, actor, critic, vn, _ = TT.setup("valuenorm", node_form="table", adj_form="none")
    _, eb, bb, _, _, _, _ = TT.setup("valuenorm", node_form="table", adj_form="none")
    assert bb._node_obs is None and bb._adj is None and bb.entity_table is not None
    cap = policy.CapturedRollout(actor, critic, bb, vn)
    for ep in range(2):
        policy.rollout(actor, critic, ba, vn)
        cap.replay()
        torch.cuda.synchronize()
        dn = ba.dones.bool()
        assert bool(dn.any()) and not bool(dn.all())
        for k in TT.STORED + ("advantages", "entity_table"):
            _same(getattr(ba, k), getattr(bb, k), "episode %d %s" % (ep, k))
        assert ba.step == bb.step == 0 and ba.act_draw == bb.act_draw == (ep + 1) * TT.T
        for b in (ba, bb):
            b.after_update()
    _same_states(ea, eb, "table-only")
    _close((ea, eb))


# ------------------------------------------------------------------------------------------------ 8: deterministic
def test_deterministic_replays_the_deterministic_rollout():
    cfg, engines, (ba, bb), actor, critic, vn = _setup(**CASES["recurrent-valuenorm-cent"])
    cap = policy.CapturedRollout(actor, critic, bb, vn, deterministic=True)
    policy.rollout(actor, critic, ba, vn, deterministic=True)
    cap.replay()
    _compare(ba, bb, "deterministic")
    # the same start sampled gives other actions: the flag is in the graph
    cfg2, engines2, (bc,), _, _, _ = _setup(buffers=1, **CASES["recurrent-valuenorm-cent"])
    policy.rollout(actor, critic, bc, vn)
    assert not torch.equal(bc.actions, bb.actions)
    _close(engines + engines2)


def test_a_construction_that_fails_half_way_changes_nothing():
    """the critic's v_out refuses in the first step of the warm-up, after the actor's chain has run, sampled into actions[0] and advanced the counter"""
    cfg, engines, (ba, bb), actor, critic, vn = _setup(**CASES["recurrent-valuenorm-cent"])
    policy.rollout(actor, critic, bb, vn)
    bb.after_update()
    bb.act_draw_counter()
    before = _snapshot(bb, engines[1], actor, critic, vn)
    counter = bb._act_draw_dev.clone()
    good, critic.v_out = critic.v_out, torch.nn.Linear(64, 2).to(DEV)
    try:
        with pytest.raises(NotImplementedError, match="2 output rows"):
            policy.CapturedRollout(actor, critic, bb, vn)
    finally:
        critic.v_out = good
    _unchanged(before, _snapshot(bb, engines[1], actor, critic, vn), "a construction that failed")
    assert torch.equal(counter, bb._act_draw_dev) and bb.step == 0 and bb.act_draw == T
    # ... and the buffer goes on as its eager twin does
    policy.rollout(actor, critic, ba, vn)
    ba.after_update()
    policy.rollout(actor, critic, ba, vn)
    policy.CapturedRollout(actor, critic, bb, vn).replay()
    _compare(ba, bb, "after the failed construction")
    _close(engines)


def test_a_step_captured_with_timing_enabled_records_no_event_pair():
    """gmpe_step asks its stream: inside a caller's capture the per-launch event pair is left out, so timing_read counts eager launches only and
    never meets an event that was recorded into a graph; the captured step is the eager step"""
    from gmpe.engine import GmpeEngine
    cfg = gmpe.make_config(num_envs=N, num_agents=A, episode_length=6, seed=11)
    eng, twin = GmpeEngine(cfg, device=0), GmpeEngine(cfg, device=0)
    act = torch.full((N, A), 3, dtype=torch.int32, device=DEV)
    for e in (eng, twin):
        e.reset()
        e.step(act)                                         # the kernel is loaded before anything is captured
    eng.timing(True)
    eng.timing_read()
    eng.step(act)
    assert eng.timing_read()[1] == 1
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.step(act)
    assert eng.timing_read()[1] == 0                        # nothing was recorded under capture (and nothing ran)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert eng.timing_read()[1] == 0
    eng.step(act)
    ms, launches = eng.timing_read()
    assert launches == 1 and ms > 0
    eng.timing(False)
    for _ in range(4):
        twin.step(act)
    torch.cuda.synchronize()
    for k in ("obs", "node_obs", "adj", "reward", "done"):
        _same(getattr(eng.out, k), getattr(twin.out, k), "captured step, " + k)
    _same_states(eng, twin, "a step captured with timing enabled")
    _close((eng, twin))


# ------------------------------------------------------------------------------------------------ 9: run(captured=True)
def test_run_captured_is_run_in_place_bit_for_bit():
    a, b = TI._setup(), TI._setup()
    b.actor.load_state_dict(a.actor.state_dict()), b.critic.load_state_dict(a.critic.state_dict())
    episodes = 3
    seen = {}
    for s, kw in ((a, dict(install="in_place")), (b, dict(captured=True))):
        got = seen[id(s)] = {"save": [], "log": [], "eval": []}
        torch.manual_seed(4)
        got["last"] = policy.run(s.actor, s.critic, s.aopt, s.copt, s.buf, s.args, s.vn, episodes=episodes, eval_engine=s.eval_eng,
                                 on_save=got["save"].append, on_log=lambda *p, got=got: got["log"].append(p),
                                 on_eval=lambda *p, got=got: got["eval"].append(p), **kw)
    torch.cuda.synchronize()
    want, got = seen[id(a)], seen[id(b)]
    assert got["save"] == want["save"] == [0, 2, 2]
    assert [p[0] for p in got["log"]] == [p[0] for p in want["log"]] == [TI.T_ROLL * TI.N_ENVS, 3 * TI.T_ROLL * TI.N_ENVS]
    assert [p[0] for p in got["eval"]] == [p[0] for p in want["eval"]] and len(got["eval"]) == 2
    for (_, ti, ei), (_, tw, ew) in zip(got["log"], want["log"]):
        assert list(ti) == list(tw) == list(policy.TRAIN_INFO) + ["average_episode_rewards"]
        for k in ti:
            _same0(ti[k], tw[k], "train_infos " + k)
        assert list(ei) == list(ew) and all(torch.equal(ei[k], ew[k]) for k in ei)
    for (_, e1), (_, e2) in zip(got["eval"], want["eval"]):
        assert all(torch.equal(e1[k], e2[k]) for k in ("eval_average_episode_rewards", "mean"))
    assert list(got["last"]) == list(want["last"])
    for k in want["last"]:
        _same0(got["last"][k], want["last"][k], "the returned train_infos " + k)
        assert bool(torch.isfinite(got["last"][k]))
    # parameters, Adam moments and step counts, learning rates, the normaliser, the buffers and the engines
    for na, nb in ((a.actor, b.actor), (a.critic, b.critic)):
        for (k, p), (_, q) in zip(na.named_parameters(), nb.named_parameters()):
            _same(p.detach(), q.detach(), k)
    for oa, ob in ((a.aopt, b.aopt), (a.copt, b.copt)):
        assert [g["lr"] for g in oa.param_groups] == [g["lr"] for g in ob.param_groups]
        assert len(oa.state) == len(ob.state) > 20
        for sa, sb in zip(oa.state.values(), ob.state.values()):
            assert float(sa["step"]) == float(sb["step"]) == 4 * episodes
            _same(sa["exp_avg"], sb["exp_avg"], "exp_avg")
            _same(sa["exp_avg_sq"], sb["exp_avg_sq"], "exp_avg_sq")
    for k in ("running_mean", "running_mean_sq", "debiasing_term"):
        _same0(getattr(a.vn, k), getattr(b.vn, k), k)
    assert a.aopt.param_groups[0]["lr"] == a.args.lr - (a.args.lr * (2 / float(3))) != a.args.lr
    for k in STORED:
        _same(getattr(a.buf, k), getattr(b.buf, k), "the buffers' " + k)
    assert a.buf.act_draw == b.buf.act_draw == episodes * TI.T_ROLL and a.buf.step == b.buf.step == 0
    _same_states(a.eng, b.eng, "run")
    TI._close(a, b)


# ------------------------------------------------------------------------------------------------ 10: refusals
def test_refusals_leave_the_engine_clean():
    cfg, engines, (ba, bb), actor, critic, vn = _setup(**CASES["recurrent-valuenorm-cent"])
    eng = engines[1]
    # a buffer in mid-episode, at construction and at replay
    cap = policy.CapturedRollout(actor, critic, bb, vn)
    policy.collect_step(actor, critic, bb)
    with pytest.raises(ValueError, match="CapturedRollout starts at buffer.step == 0, not 1"):
        policy.CapturedRollout(actor, critic, bb, vn)
    with pytest.raises(ValueError, match="CapturedRollout.replay starts at buffer.step == 0, not 1"):
        cap.replay()
    for _ in range(T - 1):
        policy.collect_step(actor, critic, bb)
    policy.compute(critic, bb, vn)
    bb.after_update()
    # timing enabled, at construction and at replay; disabled again, the replay runs
    eng.timing(True)
    before = _snapshot(bb, eng, actor, critic, vn)
    with pytest.raises(NotImplementedError, match="CapturedRollout: the engine's timing is enabled.*not supported under capture"):
        policy.CapturedRollout(actor, critic, bb, vn)
    with pytest.raises(NotImplementedError, match="CapturedRollout.replay: the engine's timing is enabled"):
        cap.replay()
    eng.timing(False)
    # a control override installed after capture
    ctrl = torch.zeros((N, A, 2), dtype=torch.float64, device=DEV)
    eng.set_control_override(ctrl)
    with pytest.raises(NotImplementedError, match="CapturedRollout.replay: the engine's control override was set or removed after capture"):
        cap.replay()
    eng.set_control_override(None)
    _unchanged(before, _snapshot(bb, eng, actor, critic, vn), "refused constructions and replays")
    # the twin catches up eagerly; then the replay is the eager rollout again
    policy.rollout(actor, critic, ba, vn)
    ba.after_update()
    policy.rollout(actor, critic, ba, vn)
    cap.replay()
    _compare(ba, bb, "after the refusals")
    # a missing normaliser, and the captured=True combinations of run
    with pytest.raises(ValueError, match="CapturedRollout: args.use_valuenorm / use_popart is set, so a value_normalizer is required"):
        policy.CapturedRollout(actor, critic, bb, None)
    opts = [torch.optim.Adam(net.parameters(), lr=1e-3) for net in (actor, critic)]
    run = lambda **kw: policy.run(actor, critic, opts[0], opts[1], bb, bb.args, vn, episodes=1, captured=True, **kw)
    with pytest.raises(NotImplementedError, match="install = 'replace': run with captured=True"):
        run(install="replace")
    with pytest.raises(NotImplementedError, match="shards: run with captured=True"):
        run(shards=types.SimpleNamespace(exchange=lambda x: x, world=1, rank=0))
    with pytest.raises(NotImplementedError, match="graph = 'table': run with captured=True"):
        run(graph="table")
    _close(engines)
