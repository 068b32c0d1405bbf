"""gmpe_env_infos / gmpe_eval_step / gmpe_eval_mean and what gmpe.infos and gmpe.policy build on them, on the device, bit for bit against
tests/infos_lib.py's restatement of float64 NumPy (tests/test_infos_host.py holds that restatement to np.mean and to the reference's recorded results):
  - gmpe_env_infos through its C entry on synthetic tensors over the sizes at which the summation takes another path (fewer than 8 values, one leaf,
    a split chunk, exactly one chunk, a second chunk of 7 values, three chunks), with guard bytes, a side stream, a repeated call, a column of all -1
    times and one NaN;
  - gmpe_eval_step and gmpe_eval_mean on the reference's recorded six steps, `first` on a dirty buffer;
  - env_infos(buffer) after a rollout and eval_episode against the same loop with host-side NumPy bookkeeping, at 8 envs x 3 agents, T = 6;
  - run over 3 episodes against the hand-written loop of iteration plus manual lr updates, waiting for nothing."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import gmpe
import gnn_lib as G
import infos_lib as IL
import trainer_lib as TL
from gmpe import _lib, infos, policy
from test_gpu_policy import DEV, K, _Net

pytestmark = pytest.mark.gpu
KEYS = 18
GUARD = 64


def synthetic_info(N, A, seed):
    rng = np.random.RandomState(seed)
    x = (rng.standard_normal((N, A, KEYS)) * np.exp(rng.uniform(-6.0, 6.0, (N, A, KEYS)))).astype(np.float32)
    ttg = np.abs(x[..., 2]) + np.float32(0.1)
    ttg[rng.rand(N, A) < 0.3] = -1.0
    ttg[:, 0] = -1.0                                         # agent 0: a column of all -1 times
    x[..., 2] = ttg
    x[N // 2, A - 1, 5] = np.nan                             # one NaN: its column alone is NaN
    return x


@pytest.mark.parametrize("A", [1, 3, 10])
@pytest.mark.parametrize("N", [1, 7, 8, 129, 1031, 8192, 8199, 16391])
def test_env_infos_entry_is_numpys_mean_bit_for_bit(N, A):
    lib = _lib.load()
    T, dt = 25, 0.1
    host = synthetic_info(N, A, 100 * A + N % 97)
    want = IL.info_means(host, T, dt)
    info = torch.from_numpy(host).to(DEV)
    raw = torch.full((GUARD + A * KEYS * 8 + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    assert raw.data_ptr() % 8 == 0
    out_ptr = raw.data_ptr() + GUARD
    plan = _lib.GmpeEnvInfosPlan(N, A, T, 0, dt, info.data_ptr(), out_ptr)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    got = []
    for _ in range(2):                                       # a repeated call gives the same bits
        with torch.cuda.stream(side):
            _lib.check(lib.gmpe_env_infos(0, C.byref(plan), C.c_void_p(side.cuda_stream)), "gmpe_env_infos")
        side.synchronize()
        b = raw.cpu().numpy()
        assert (b[:GUARD] == 0xFF).all() and (b[-GUARD:] == 0xFF).all()
        got.append(b[GUARD:-GUARD].copy().view(np.float64).reshape(A, KEYS))
    assert IL.same_bits(got[0], got[1])
    assert IL.same_bits(got[0], want), np.argwhere(IL.bits(got[0]) != IL.bits(want))[:5]
    nan = np.isnan(got[0])
    assert nan.sum() == 1 and nan[A - 1, 5]
    # the all -1 column: a mean of N equal values, rounded as NumPy rounds it
    assert IL.same_bits(got[0][0, 2], IL.np_mean(np.full(N, np.float64(T) * np.float64(dt))))


def test_eval_step_and_mean_on_the_references_six_steps():
    fx = IL.load()
    rewards, dones, rnn_out = fx["eval/rewards"], fx["eval/dones"], fx["eval/rnn_out"]
    T, N, A = rewards.shape
    H = rnn_out.shape[-1]
    for with_rnn in (True, False):
        sums = torch.full((N, A), float("nan"), dtype=torch.float64, device=DEV)        # dirty: `first` stores
        masks = torch.full((N, A, 1), 7.0, dtype=torch.float32, device=DEV)
        rnn = torch.zeros((N, A, 1, H), dtype=torch.float32, device=DEV) if with_rnn else None
        for t in range(T):
            if with_rnn:
                rnn.copy_(torch.from_numpy(rnn_out[t]).view(N, A, 1, H))                # what act returned
            infos.eval_step(torch.from_numpy(rewards[t].astype(np.float32)).to(DEV), torch.from_numpy(dones[t]).to(DEV), sums, masks, rnn, first=t == 0)
            if t + 1 < T:
                assert np.array_equal(masks.cpu().numpy().reshape(N * A, 1), fx["eval/masks_in"][t + 1]), t
                if with_rnn:
                    assert np.array_equal(rnn.cpu().numpy().reshape(N * A, 1, H), fx["eval/rnn_in"][t + 1]), t
        assert IL.same_bits(sums.cpu().numpy(), fx["eval/sums"])
        mean = infos.eval_mean(sums)
        assert mean.dim() == 0 and mean.dtype == torch.float64 and IL.same_bits(mean.cpu().numpy(), fx["eval/mean"])


@pytest.mark.parametrize("count", [1, 7, 129, 8199 * 3, 40960])
def test_eval_mean_is_numpys_mean_bit_for_bit(count):
    rng = np.random.RandomState(count)
    x = rng.standard_normal(count) * np.exp(rng.uniform(-8.0, 8.0, count))
    raw = torch.full((GUARD + 8 + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    out = raw[GUARD:GUARD + 8].view(torch.float64).view(())
    got = infos.eval_mean(torch.from_numpy(x).to(DEV), out=out)
    assert got.data_ptr() == out.data_ptr() and IL.same_bits(got.cpu().numpy(), IL.np_mean(x))
    b = raw.cpu().numpy()
    assert (b[:GUARD] == 0xFF).all() and (b[-GUARD:] == 0xFF).all()


# ------------------------------------------------------------------------------------------------ engine-driven: 8 envs x 3 agents, T = 6
N_ENVS, AGENTS, T_ROLL = 8, 3, 6


class _ValueNorm(TL.ValueNorm):
    def running_mean_var(self):                             # valuenorm.py:48-55
        mean = self.running_mean / self.debiasing_term.clamp(min=self.epsilon)
        return mean, (self.running_mean_sq / self.debiasing_term.clamp(min=self.epsilon) - mean ** 2).clamp(min=1e-2)


def _args():
    return types.SimpleNamespace(
        gamma=0.99, gae_lambda=0.95, use_gae=True, use_proper_time_limits=False, use_valuenorm=True, use_popart=False, clip_param=0.2, huber_delta=10.0,
        entropy_coef=0.01, use_policy_active_masks=True, use_value_active_masks=True, use_clipped_value_loss=True, use_huber_loss=True,
        use_max_grad_norm=True, max_grad_norm=0.5, value_loss_coef=0.5, use_recurrent_policy=True, use_naive_recurrent_policy=False, ppo_epoch=2,
        num_mini_batch=2, data_chunk_length=3, recurrent_N=1, hidden_size=64, episode_length=T_ROLL, n_rollout_threads=N_ENVS, save_interval=2,
        log_interval=2, eval_interval=2, use_eval=True, use_linear_lr_decay=True, lr=5e-4, critic_lr=7e-4)


def _setup(seed=11):
    """an engine with a buffer, an eval engine, the shipped-weight actor and a critic, their optimisers, the value normaliser"""
    from gmpe.engine import GmpeEngine
    from gmpe.rollout import DeviceRolloutBuffer
    cfg = gmpe.make_config(num_envs=N_ENVS, num_agents=AGENTS, episode_length=4, seed=seed)      # the time limit lies inside the rollout: dones occur
    eng, eval_eng = GmpeEngine(cfg, device=0), GmpeEngine(gmpe.make_config(num_envs=N_ENVS, num_agents=AGENTS, episode_length=4, seed=seed + 1), device=0)
    key = G.ACTOR if int(cfg.node_feats) == 7 else G.ROTATE
    assert int(cfg.n_actions) == K
    actor = _Net(key, eng.D, "act").to(DEV)
    critic = _Net(key, eng.D, "v_out", use_cent_obs=True, seed=12).to(DEV)
    vn = _ValueNorm(DEV)
    vn.running_mean.fill_(0.3), vn.running_mean_sq.fill_(0.7), vn.debiasing_term.fill_(0.5)
    args = _args()
    buf = DeviceRolloutBuffer(eng, T_ROLL, use_centralized_V=False, policy_fields="all", learner_fields="all", args=args, recurrent_N=1, hidden_size=64)
    adam = lambda net, lr: torch.optim.Adam(net.parameters(), lr=lr, eps=1e-5)
    return types.SimpleNamespace(cfg=cfg, eng=eng, eval_eng=eval_eng, actor=actor, critic=critic, vn=vn, args=args, buf=buf,
                                 aopt=adam(actor, args.lr), copt=adam(critic, args.critic_lr))


def _close(*setups):
    for s in setups:
        for e in (s.eng, s.eval_eng):
            e.check_errors()
            e.close()


def _host(d):
    return {k: v.detach().cpu().numpy().copy() for k, v in d.items()}


def _eval_by_hand(actor, eng, T, seed):
    """eval_episode's loop with the reference's NumPy bookkeeping on the host around the same actor_forward calls"""
    N, A = eng.N, eng.A
    rows = N * A
    o = eng.reset()
    E = int(o.node_obs.shape[-2])
    rnn, masks = np.zeros((N, A, 1, 64), dtype=np.float32), np.ones((N, A, 1), dtype=np.float32)
    rewards = []
    for t in range(T):
        idx, _, h = policy.actor_forward(actor, o.obs.reshape(rows, -1), o.node_obs.reshape(rows, E, -1), o.adj.reshape(-1, E, E), o.agent_id.reshape(rows),
                                         torch.from_numpy(rnn).to(DEV).view(rows, 1, 64), torch.from_numpy(masks).to(DEV).view(rows, 1), None, True,
                                         seed=seed, env_id_base=int(eng.cfg.env_id_base), num_agents=A, draw=t, out={})
        rnn = h.cpu().numpy().reshape(N, A, 1, 64).copy()
        o = eng.step(idx.view(N, A))
        rewards.append(o.reward.cpu().numpy().astype(np.float64))
        dones_env = np.all(o.done.cpu().numpy().astype(bool), axis=1)
        rnn[dones_env] = 0.0
        masks = np.ones((N, A, 1), dtype=np.float32)
        masks[dones_env] = 0.0
    sums = np.sum(np.array(rewards), axis=0)
    return sums, IL.np_mean(sums), np.array(rewards)


def test_env_infos_of_a_rollout_and_eval_episode_are_the_loops_written_out():
    s = _setup()
    s.buf.warmup()
    policy.rollout(s.actor, s.critic, s.buf, s.vn)
    got = infos.env_infos(s.buf)
    for source in (s.eng, s.buf.info):
        again = infos.env_infos(source, episode_length=T_ROLL, dt=float(s.cfg.dt), include_min_time=s.cfg.max_speed > 0)
        assert list(again) == list(got) and all(torch.equal(again[k], got[k]) for k in got)
    want = IL.env_infos(s.buf.info.cpu().numpy(), T_ROLL, float(s.cfg.dt), include_min_time=s.cfg.max_speed > 0)
    assert list(got) == list(want) and len(got) == AGENTS * (16 + int(s.cfg.max_speed > 0))
    base = next(iter(got.values()))
    assert all(v.dim() == 0 and v.dtype == torch.float64 and v.device.type == "cuda" and v.untyped_storage().data_ptr() == base.untyped_storage().data_ptr()
               for v in got.values())                       # views of one [A, 18] result
    assert IL.same_bits(np.array([v.item() for v in got.values()]), np.array(list(want.values())))
    assert len(set(float(v) for v in want.values())) > AGENTS * 4
    # eval_episode against the same loop with host-side bookkeeping, on two engines of one config
    ev = policy.eval_episode(s.actor, s.eval_eng, s.args, seed=5)
    assert list(ev) == ["eval_average_episode_rewards", "mean"]
    sums, mean = ev["eval_average_episode_rewards"], ev["mean"]
    assert tuple(sums.shape) == (N_ENVS, AGENTS) and sums.dtype == torch.float64 and mean.dim() == 0 and mean.dtype == torch.float64
    from gmpe.engine import GmpeEngine
    hand_eng = GmpeEngine(s.eval_eng.cfg, device=0)          # the same envs from the same start
    want_sums, want_mean, rewards = _eval_by_hand(s.actor, hand_eng, T_ROLL, 5)
    hand_eng.check_errors()
    hand_eng.close()
    assert IL.same_bits(sums.cpu().numpy(), want_sums) and IL.same_bits(mean.cpu().numpy(), want_mean)
    assert np.unique(rewards).size > T_ROLL * N_ENVS        # an episode did play, with the time limit of 4 inside it
    _close(s)


def test_run_is_the_hand_written_loop_and_waits_for_nothing():
    a, b = _setup(), _setup()
    b.actor.load_state_dict(a.actor.state_dict()), b.critic.load_state_dict(a.critic.state_dict())
    episodes = 3
    for s in (a, b):                                        # warm: every kernel loaded, every optimiser state created, alike on both
        s.buf.warmup()
        torch.manual_seed(3)
        policy.iteration(s.actor, s.critic, s.aopt, s.copt, s.buf, s.args, s.vn, value_head="device")
        policy.eval_episode(s.actor, s.eval_eng, s.args, seed=0)
        infos.env_infos(s.buf, s.args)
    got = {"save": [], "log": [], "eval": []}
    one = torch.ones((), device=DEV)
    torch.cuda.synchronize()
    torch.manual_seed(4)
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            one.item()
        last = policy.run(a.actor, a.critic, a.aopt, a.copt, a.buf, a.args, a.vn, episodes=episodes, eval_engine=a.eval_eng, value_head="device",
                          on_save=got["save"].append, on_log=lambda *p: got["log"].append(p), on_eval=lambda *p: got["eval"].append(p))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    # the same by hand
    want = {"save": [], "log": [], "eval": []}
    torch.manual_seed(4)
    b.buf.warmup()
    for ep in range(episodes):
        for opt, lr0 in ((b.aopt, b.args.lr), (b.copt, b.args.critic_lr)):
            for g in opt.param_groups:
                g["lr"] = lr0 - (lr0 * (ep / float(episodes)))
        info = policy.iteration(b.actor, b.critic, b.aopt, b.copt, b.buf, b.args, b.vn, value_head="device")
        steps = (ep + 1) * T_ROLL * N_ENVS
        if ep % 2 == 0 or ep == episodes - 1:
            want["save"].append(ep)
        if ep % 2 == 0:
            want["log"].append((steps, info, IL.env_infos(b.buf.info.cpu().numpy(), T_ROLL, float(b.cfg.dt), include_min_time=b.cfg.max_speed > 0)))
        if ep % 2 == 0:
            want["eval"].append((steps, policy.eval_episode(b.actor, b.eval_eng, b.args, seed=0)))
    want["save"].append(episodes - 1)
    torch.cuda.synchronize()
    assert got["save"] == want["save"] == [0, 2, 2]
    assert [p[0] for p in got["log"]] == [p[0] for p in want["log"]] == [T_ROLL * N_ENVS, 3 * T_ROLL * N_ENVS]
    assert [p[0] for p in got["eval"]] == [p[0] for p in want["eval"]]
    for (_, ti, ei), (_, tw, ew) in zip(got["log"], want["log"]):
        assert list(ti) == list(tw) == list(policy.TRAIN_INFO) + ["average_episode_rewards"]
        assert all(torch.equal(ti[k], tw[k]) for k in ti)
        assert list(ei) == list(ew) and IL.same_bits(np.array([v.item() for v in ei.values()]), np.array(list(ew.values())))
    for (_, e1), (_, e2) in zip(got["eval"], want["eval"]):
        assert all(torch.equal(e1[k], e2[k]) for k in ("eval_average_episode_rewards", "mean"))
    assert all(torch.equal(last[k], info[k]) for k in info)
    # parameters, Adam state, normaliser and learning rates, bit for bit
    for na, nb in ((a.actor, b.actor), (a.critic, b.critic)):
        assert all(torch.equal(p, q) for p, q in zip(na.parameters(), nb.parameters()))
    for oa, ob in ((a.aopt, b.aopt), (a.copt, b.copt)):
        assert [g["lr"] for g in oa.param_groups] == [g["lr"] for g in ob.param_groups]
        for sa, sb in zip(oa.state.values(), ob.state.values()):
            assert float(sa["step"]) == float(sb["step"]) == 4 * (episodes + 1)
            assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"])
    for k in ("running_mean", "running_mean_sq", "debiasing_term"):
        assert torch.equal(getattr(a.vn, k), getattr(b.vn, k)), k
    assert a.aopt.param_groups[0]["lr"] == a.args.lr - (a.args.lr * (2 / float(3))) != a.args.lr
    _close(a, b)
