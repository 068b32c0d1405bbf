"""Host side of gmpe.infos and of gmpe.policy.run / eval_episode. No GPU.
  - tests/infos_lib.py's restatement of NumPy's summation order equals np.mean / np.add.reduce exactly, and plain pairwise recursion without the
    8192-element chunks does not (the mutant that keeps this test honest): a NumPy whose reduce buffer differs fails here, so the GPU tests need not ask;
  - the bounds gmpe_infos.hip's split-tree program is built for hold for every chunk size;
  - the restatements of process_infos + log_env and of eval reproduce the reference's recorded results (tests/golden/run_log.npz): names, order,
    absent keys, values, masks, zeroed rows — and the package's own key table is that order;
  - every refusal is by name, Python and C, with fake aligned pointers and no device;
  - run's schedule: callbacks, total_num_steps and learning rates over 5 episodes with intervals 2 / 2 / 3."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import infos_lib as IL
from gmpe import _lib, config as gcfg, infos, policy

SIZES = [1, 7, 8, 9, 127, 128, 129, 136, 257, 1031, 8191, 8192, 8193, 12000, 16385, 40960]


def draws(n, seed):
    rng = np.random.RandomState(seed)
    return [(rng.standard_normal(n) * np.exp(rng.uniform(-8.0, 8.0, n))).astype(np.float32).astype(np.float64) for _ in range(5)]


@pytest.mark.parametrize("n", SIZES)
def test_the_restatement_is_numpys_order(n):
    for x in draws(n, 1000 + n):
        assert IL.same_bits(IL.np_sum(x), np.add.reduce(x)), n
        assert IL.same_bits(IL.np_mean(x), np.mean(x)) and IL.same_bits(IL.np_mean(x), np.mean(x.tolist())), n


def test_the_column_form_is_the_same_adds():
    x = np.stack(draws(8192 + 300, 77), axis=1)
    assert IL.same_bits(IL.np_mean_columns(x), np.array([IL.np_mean(x[:, c]) for c in range(x.shape[1])]))


def test_negative_zero_and_nan_follow_numpy():
    for x in ([-0.0], [-0.0] * 9, [-0.0] * 200, [0.0, -0.0]):
        assert IL.same_bits(IL.np_mean(x), np.mean(x)), x
    x = draws(300, 5)[0]
    x[131] = np.nan
    assert np.isnan(IL.np_mean(x)) and np.isnan(np.mean(x))


def test_plain_recursion_without_chunks_is_not_numpys_order():
    xs = draws(12000, 1000 + 12000)
    assert sum(not IL.same_bits(IL.np_sum(x, chunk=None), np.add.reduce(x)) for x in xs) >= 1
    assert all(IL.same_bits(IL.np_sum(x, chunk=None), np.add.reduce(x)) for x in draws(8192, 1000 + 8192))      # one chunk: the same order


def test_the_split_trees_fit_the_kernels_tables():
    """gmpe_infos.hip holds a chunk's tree in LDS: at most CHUNK / (LEAF / 2) leaves, twice as many tokens, a stack of 16"""
    assert (_lib.INFOS_CHUNK, _lib.INFOS_LEAF) == (IL.CHUNK, IL.LEAF)
    worst_leaves = worst_depth = 0
    for m in list(range(1, 1200)) + list(range(1200, IL.CHUNK + 1, 7)) + [IL.CHUNK - 1, IL.CHUNK]:
        lv, depth = IL.leaves(m)
        assert sum(n for _, n in lv) == m and all(0 < n <= IL.LEAF for _, n in lv)
        worst_leaves, worst_depth = max(worst_leaves, len(lv)), max(worst_depth, depth)
    assert worst_leaves <= IL.CHUNK // (IL.LEAF // 2) and worst_depth <= 8, (worst_leaves, worst_depth)


def fixture_info(fx, n):
    return fx["infos/8200/pool"][fx["infos/8200/index"]] if n == 8200 else fx["infos/%d/info" % n]


@pytest.mark.parametrize("n", [5, 130, 8200])
def test_the_restatement_reproduces_process_infos_and_log_env(n):
    fx = IL.load()
    info = fixture_info(fx, n)
    assert info.shape == (n, 3, 18) and info.dtype == np.float32 and (info[..., 2] == -1).any()
    T, dt, min_time = int(fx["infos/%d/episode_length" % n]), float(fx["infos/%d/dt" % n]), bool(fx["infos/%d/min_time" % n])
    got = IL.env_infos(info, T, dt, include_min_time=min_time)
    names = [str(k) for k in fx["infos/%d/names" % n]]
    assert list(got) == names
    assert IL.same_bits(np.array(list(got.values())), fx["infos/%d/values" % n])
    # absent keys: formation_dist and Phase_reached never, min_time_to_goal only with max_speed
    assert not any("formation_dist" in k or "hase" in k for k in names) and any("min_time_to_goal" in k for k in names) == min_time
    assert names[:4] == ["agent0/individual_rewards", "agent0/time_to_goal"] + (["agent0/min_time_to_goal"] if min_time else []) + ["agent0/dist_to_goal"] \
        + ([] if min_time else ["agent0/num_agent_collisions"])
    # the package's key table is that order, and its columns are config.INFO_KEYS'
    assert [k for k, _, _ in infos.env_info_keys(3, min_time)] == names
    assert IL.INFO_KEYS == list(gcfg.INFO_KEYS) == [str(k) for k in fx["info_keys"]]
    # without the -1 rule the values differ: the fixture does exercise it
    assert not IL.same_bits(np.array(list(IL.env_infos(info, T, dt * 2, min_time).values())), fx["infos/%d/values" % n])


def test_the_restatement_reproduces_eval():
    fx = IL.load()
    rewards, dones, rnn_out = fx["eval/rewards"], fx["eval/dones"], fx["eval/rnn_out"]
    T, N, A = rewards.shape
    assert str(fx["eval/reward_dtype"]) == "float64" and rewards.dtype == np.float64
    assert IL.same_bits(rewards, rewards.astype(np.float32))                    # float32 values widened: the device's rewards can be these
    sums, mean, masks, zeroed = IL.eval_episode(rewards, dones)
    assert IL.same_bits(sums, fx["eval/sums"]) and IL.same_bits(mean, fx["eval/mean"])
    masks_in, rnn_in = fx["eval/masks_in"], fx["eval/rnn_in"]
    assert (masks_in[0] == 1).all() and (rnn_in[0] == 0).all()
    for t in range(T - 1):
        assert np.array_equal(masks_in[t + 1], masks[t].reshape(N * A, 1)), t
        want = rnn_out[t].reshape(N, A, -1).copy()
        want[zeroed[t]] = 0.0
        assert np.array_equal(rnn_in[t + 1].reshape(N, A, -1), want), t
    # the pattern: an env that finishes early, one whose single done agent resets nothing, one that finishes on the last step
    assert zeroed[1, 0] and not zeroed[:, 1].any() and dones[2:, 1, 1].all() and zeroed[T - 1, 2] and not zeroed[:T - 1, 2].any()
    assert (masks[2][1] == 1).all()                                             # per env, not per agent


# ------------------------------------------------------------------------------------------------ refusals
FAKE = 0x10000


def c_error(fn, plan):
    lib = _lib.load()
    rc = getattr(lib, fn)(0, C.byref(plan) if plan is not None else None, None)
    assert rc == -1, (fn, rc)
    text = lib.gmpe_last_error().decode()
    assert text.startswith(fn + ": "), text
    return text


def test_c_entries_refuse_by_name_before_any_launch():
    good = dict(num_envs=4, num_agents=3, episode_length=25, reserved=0, dt=0.1, info=FAKE, out=FAKE)
    for field, value, word in (("num_envs", 0, "num_envs"), ("num_agents", 0, "num_agents"), ("num_agents", 65, "num_agents"),
                               ("episode_length", 0, "episode_length"), ("reserved", 1, "reserved"), ("dt", float("nan"), "dt"),
                               ("dt", float("inf"), "dt"), ("info", None, "info"), ("out", None, "out"), ("info", FAKE + 2, "info"),
                               ("out", FAKE + 4, "out")):
        assert word in c_error("gmpe_env_infos", _lib.GmpeEnvInfosPlan(**dict(good, **{field: value}))), field
    assert "null plan" in c_error("gmpe_env_infos", None)
    good = dict(num_envs=4, num_agents=3, rnn_row=64, first=0, reward=FAKE, done=FAKE + 1, sums=FAKE, masks=FAKE, rnn_states=FAKE)
    for field, value, word in (("num_envs", 0, "num_envs"), ("num_agents", 65, "num_agents"), ("first", 2, "first"), ("rnn_row", 0, "rnn_row"),
                               ("rnn_row", (1 << 20) + 1, "rnn_row"), ("reward", None, "reward"), ("done", None, "done"), ("sums", None, "sums"),
                               ("masks", None, "masks"), ("reward", FAKE + 2, "reward"), ("sums", FAKE + 4, "sums"), ("masks", FAKE + 1, "masks"),
                               ("rnn_states", FAKE + 2, "rnn_states")):
        assert word in c_error("gmpe_eval_step", _lib.GmpeEvalStepPlan(**dict(good, **{field: value}))), field
    assert "rnn_row" in c_error("gmpe_eval_step", _lib.GmpeEvalStepPlan(**dict(good, rnn_states=None)))      # a row size without states
    assert "null plan" in c_error("gmpe_eval_step", None)
    good = dict(count=12, values=FAKE, out=FAKE)
    for field, value, word in (("count", 0, "count"), ("count", (1 << 40) + 1, "count"), ("values", None, "values"), ("out", None, "out"),
                               ("values", FAKE + 4, "values"), ("out", FAKE + 4, "out")):
        assert word in c_error("gmpe_eval_mean", _lib.GmpeEvalMeanPlan(**dict(good, **{field: value}))), field
    assert "null plan" in c_error("gmpe_eval_mean", None)


def test_python_refuses_by_name_without_a_device():
    cfg = types.SimpleNamespace(dt=0.1, max_speed=2.0, episode_length=25, env_id_base=0)
    no_info = types.SimpleNamespace(out=types.SimpleNamespace(info=None, node_obs=None, adj=None), cfg=cfg, N=4, A=3)
    with pytest.raises(ValueError, match="engine.out.info is None.*without info"):
        infos.env_infos(no_info)
    with pytest.raises(ValueError, match="buffer.info is None.*without info"):
        infos.env_infos(types.SimpleNamespace(info=None, engine=no_info, T=6))
    with pytest.raises(ValueError, match="source must be a DeviceRolloutBuffer"):
        infos.env_infos(object())
    host = torch.zeros((4, 3, 18))
    with pytest.raises(ValueError, match="episode_length is required"):
        infos.env_infos(host)
    with pytest.raises(ValueError, match="dt is required"):
        infos.env_infos(host, episode_length=6)
    with pytest.raises(ValueError, match=r"must be a float32 \[N, A, 18\] tensor"):
        infos.env_infos(torch.zeros((4, 3, 17)), episode_length=6, dt=0.1)
    with pytest.raises(ValueError, match="source must be a CUDA"):
        infos.env_infos(host, episode_length=6, dt=0.1)
    with pytest.raises(ValueError, match="reward must be a CUDA"):
        infos.eval_step(torch.zeros((4, 3)), None, None, None)
    with pytest.raises(ValueError, match="values must be a CUDA"):
        infos.eval_mean(torch.zeros((4, 3), dtype=torch.float64))
    with pytest.raises(ValueError, match="eval_engine must be a GmpeEngine"):
        policy.eval_episode(None, object())
    with pytest.raises(ValueError, match="node_obs rows"):
        policy.eval_episode(None, no_info)
    args = types.SimpleNamespace(increase_fairness=True)
    with pytest.raises(NotImplementedError, match="args.increase_fairness.*not supported"):
        policy.run(None, None, None, None, None, args)
    with pytest.raises(ValueError, match="args.use_eval is set: run needs eval_engine"):
        policy.run(None, None, None, None, None, types.SimpleNamespace(use_eval=True))
    buf = types.SimpleNamespace(T=6, engine=types.SimpleNamespace(N=4))
    with pytest.raises(ValueError, match="episodes= or args.num_env_steps"):
        policy.run(None, None, None, None, buf, types.SimpleNamespace())
    with pytest.raises(ValueError, match="args.lr and args.critic_lr"):
        policy.run(None, None, None, None, buf, types.SimpleNamespace(use_linear_lr_decay=True, lr=1e-3), episodes=2)


# ------------------------------------------------------------------------------------------------ run's schedule
def test_runs_schedule_is_the_references(monkeypatch):
    events, lrs = [], []
    aopt = types.SimpleNamespace(param_groups=[{"lr": -1.0}, {"lr": -1.0}])
    copt = types.SimpleNamespace(param_groups=[{"lr": -1.0}])
    buf = types.SimpleNamespace(T=6, engine=types.SimpleNamespace(N=4), warmup=lambda: events.append("warmup"))

    def iteration(actor, critic, a, c, buffer, args, vn, **kw):
        assert (a, c, buffer, vn, kw) == (aopt, copt, buf, "vn", {"value_head": "device"})
        lrs.append((a.param_groups[0]["lr"], a.param_groups[1]["lr"], c.param_groups[0]["lr"]))
        events.append("iteration")
        return {"n": len(lrs)}

    monkeypatch.setattr(policy, "iteration", iteration)
    monkeypatch.setattr(policy._infos, "env_infos", lambda buffer, args: events.append("env_infos") or {"from": buffer})
    monkeypatch.setattr(policy, "eval_episode", lambda actor, eng, args, seed: events.append("eval_episode") or {"engine": eng, "seed": seed})
    args = types.SimpleNamespace(num_env_steps=5 * 6 * 4 + 23, episode_length=6, n_rollout_threads=4, save_interval=2, log_interval=2, eval_interval=3,
                                 use_eval=True, use_linear_lr_decay=True, lr=7e-4, critic_lr=3e-4)
    last = policy.run("actor", "critic", aopt, copt, buf, args, "vn", eval_engine="eval-engine", eval_seed=9, value_head="device",
                      on_save=lambda ep: events.append(("save", ep)),
                      on_log=lambda steps, train, env: events.append(("log", steps, train["n"], env["from"] is buf)),
                      on_eval=lambda steps, ev: events.append(("eval", steps, ev["engine"], ev["seed"])))
    assert last == {"n": 5}
    s = 24                                                   # episode_length * n_rollout_threads
    assert events == ["warmup",
                      "iteration", ("save", 0), "env_infos", ("log", s, 1, True), "eval_episode", ("eval", s, "eval-engine", 9),
                      "iteration",
                      "iteration", ("save", 2), "env_infos", ("log", 3 * s, 3, True),
                      "iteration", "eval_episode", ("eval", 4 * s, "eval-engine", 9),
                      "iteration", ("save", 4), "env_infos", ("log", 5 * s, 5, True),
                      ("save", 4)]                           # the final forced save comes after the loop
    want = [(7e-4 - (7e-4 * (ep / float(5))), 3e-4 - (3e-4 * (ep / float(5)))) for ep in range(5)]
    assert lrs == [(a, a, c) for a, c in want]
    # without callbacks nothing is computed for them, and without use_eval no eval runs; without decay the rates stay
    del events[:], lrs[:]
    args.use_eval, args.use_linear_lr_decay = False, False
    policy.run("actor", "critic", aopt, copt, buf, args, "vn", episodes=2, value_head="device", on_eval=lambda *a: events.append("eval"))
    assert events == ["warmup", "iteration", "iteration"] and lrs == [lrs[0]] * 2
