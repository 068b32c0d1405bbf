"""Golden vectors for the rollout half of gmpe.policy (get_actions, get_values, compute, the learner fields of insert), produced by RUNNING the
reference's runner on the CPU, in the build container only:

    python tests/golden/make_rollout_fixture.py        # writes tests/golden/rollout_*.npz and prints the err_ref table

What runs is the reference's own code, through make_trainer_fixture.py's harness: GR_Actor and GR_Critic (graph_actor_critic.py) with the shipped GNN
and head weights and the reference's seeded init for the rest, PopArt / ValueNorm, GraphReplayBuffer, and GMPERunner.collect (step 0),
GMPERunner.collect_with_mask (later steps, with get_finished's lists as run() forms them), GMPERunner.insert and GMPERunner.compute, used unbound on
a namespace that holds what they read. THE ONE SWAP is make_trainer_fixture.py's: gnn_new, replaced by the adapter around tests/gnn_lib.py.

The env is prescribed: T = 6 steps of seeded outputs with the shapes of an engine config of a 7-feature scenario (N = 2, A = 3; tests/rollout_lib.py),
graphs as gnn_lib draws them, so that the GPU test can replay them through a real DeviceRolloutBuffer with insert_external. The prescribed dones hold an
agent done alone mid-rollout (step 2) and a whole env done (step 3).

The policy namespace's get_actions is the two calls GR_MAPPOPolicy.get_actions makes (actor.forward, critic.forward), with deterministic=True — the
reference's mode() — because torch's sampler and the device's Philox stream cannot be matched; get_values is its one call.

Each case (valuenorm, popart) runs in float64 — modules .double(), every tpdv dtype and the buffer's float arrays in float64: the truth — and in float32
as shipped, which gives err_ref = max|a32 - a64| / max|a64|. Asserted here, the next seed taken on failure: err_ref <= 1e-5 for every stored array;
every row's top two (available) logits at least 1e-4 apart in the float64 run; every ReLU pre-activation at least 1e-5 from zero; the two runs take the
same actions. Data only is written."""
import argparse
import json
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
warnings.filterwarnings("ignore")
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import gnn_lib as G  # noqa: E402
import head_lib as HL  # noqa: E402
import make_buffer_fixture as MB  # noqa: E402
import make_trainer_fixture as MT  # noqa: E402
import rollout_lib as RL  # noqa: E402
import trainer_lib as TL  # noqa: E402

N, A, T = RL.N, RL.A, RL.T
DONES = {2: [(0, 1)], 3: [(1, 0), (1, 1), (1, 2)]}      # step -> the (env, agent) pairs done at that step


def build(REF, case, dt, seed, S):
    """the reference's actor and critic in dtype dt, its value normaliser with statistics that are not the fresh ones, and the policy namespace;
    margin[0]: the smallest |pre-activation| any ReLU saw; logits: what the actor's head gave, call by call"""
    import gym
    GR_Actor, GR_Critic, _ = REF
    sp = lambda s: gym.spaces.Box(-np.inf, np.inf, s, np.float32)
    a = types.SimpleNamespace(use_popart=case == "popart", use_valuenorm=case == "valuenorm", use_recurrent_policy=True, use_naive_recurrent_policy=False,
                              use_policy_active_masks=True)
    args = MT.ref_args(a)
    torch.manual_seed(seed)
    actor = GR_Actor(args, sp((S["D"],)), sp((S["E"], 7)), sp((1,)), gym.spaces.Discrete(S["K"]))
    critic = GR_Critic(args, sp((S["D"],)), sp((S["E"], 7)), sp((1,)))
    g = HL.golden()
    with torch.no_grad():
        actor.act.action_out.linear.weight.copy_(torch.from_numpy(g["actor.act.action_out.linear.weight"]))
        actor.act.action_out.linear.bias.copy_(torch.from_numpy(g["actor.act.action_out.linear.bias"]))
        critic.v_out.weight.copy_(torch.from_numpy(g["critic.v_out.weight"]))
        critic.v_out.bias.copy_(torch.from_numpy(g["critic.v_out.bias"]))
        if case == "popart":
            critic.v_out.stddev.copy_(torch.from_numpy(g["critic.v_out.stddev"]))
            critic.v_out.mean.fill_(-0.2), critic.v_out.mean_sq.fill_(0.9), critic.v_out.debiasing_term.fill_(0.4)
    init = {"actor": MT.state_dict(actor), "critic": MT.state_dict(critic)}
    actor, critic = actor.to(dt), critic.to(dt)
    actor.tpdv["dtype"] = critic.tpdv["dtype"] = dt
    norm = {}
    if case == "popart":
        critic.v_out.tpdv["dtype"] = dt
        vn = critic.v_out                                   # graph_mappo.py:63-64
    else:
        from onpolicy.utils.valuenorm import ValueNorm
        vn = ValueNorm(1)
        with torch.no_grad():
            vn.running_mean.fill_(0.3), vn.running_mean_sq.fill_(0.7), vn.debiasing_term.fill_(0.5)
        norm = {k: getattr(vn, k).detach().float().numpy().copy() for k in ("running_mean", "running_mean_sq", "debiasing_term")}
        vn.to(dt)
        vn.tpdv["dtype"] = dt
    margin, logits = [np.inf], []

    def seen(mod, inp):
        margin[0] = min(margin[0], float(inp[0].detach().abs().min())) if inp[0].numel() else margin[0]
    for net in (actor, critic):
        for m in set(m for m in net.modules() if isinstance(m, nn.ReLU)):
            m.register_forward_pre_hook(seen)
    actor.act.action_out.linear.register_forward_hook(lambda m, i, o: logits.append(o.detach().double().clone()))

    def get_actions(cent_obs, obs, node_obs, adj, agent_id, share_agent_id, h, hc, masks, available_actions=None, deterministic=False):
        actions, lp, h = actor(obs, node_obs, adj, agent_id, h, masks, available_actions, True)     # graph_MAPPOPolicy.py:149-156, with mode()
        values, hc = critic(cent_obs, node_obs, adj, share_agent_id, hc, masks)                     # :158-163
        return values, actions, lp, h, hc

    def get_values(cent_obs, node_obs, adj, share_agent_id, hc, masks):
        return critic(cent_obs, node_obs, adj, share_agent_id, hc, masks)[0]
    pol = types.SimpleNamespace(actor=actor, critic=critic, get_actions=get_actions, get_values=get_values)
    return pol, vn, init, norm, margin, logits


def draw_env(seed, S):
    """the prescribed env outputs: slot 0 (the reset) and T steps"""
    rng = np.random.RandomState(7000 + seed)
    D, E = S["D"], S["E"]
    env = {k: [] for k in RL.ENV}
    for t in range(T + 1):
        x, adj, ids = G.draw(rng, N * A, E, 7)
        env["obs"].append(rng.randn(N, A, D).astype(np.float32))
        env["node_obs"].append(x.reshape(N, A, E, 7))
        env["adj"].append(adj.reshape(N, A, E, E))
        env["agent_id"].append(ids.reshape(N, A, 1))
        if t:
            env["rewards"].append(rng.randn(N, A, 1).astype(np.float32))
            dn = np.zeros((N, A), bool)
            for e, a in DONES.get(t - 1, ()):
                dn[e, a] = True
            env["dones"].append(dn)
    env = {k: np.array(v) for k, v in env.items()}
    dn = env["dones"]
    assert any(dn[t].sum(1).max() == 1 and 0 < t < T - 1 for t in range(T)) and any(dn[t].all(1).any() for t in range(T)) and not dn[-1].any()
    return env


def run(REF, case, dt, seed, env, S):
    """T steps of run()'s loop (graph_mpe_runner.py:57-103) with the prescribed env in place of envs.step, then compute()"""
    GraphReplayBuffer, GMPERunner = MB.load_reference()
    import gym
    pol, vn, init, norm, margin, logits = build(REF, case, dt, seed, S)
    D, E, K = S["D"], S["E"], S["K"]
    args = argparse.Namespace(episode_length=T, n_rollout_threads=N, hidden_size=64, recurrent_N=1, use_popart=case == "popart",
                              use_valuenorm=case == "valuenorm", use_centralized_V=False, num_agents=A, **RL.RETURNS_ARGS)
    sp = lambda shape: gym.spaces.Box(-np.inf, np.inf, shape, np.float32)
    space = gym.spaces.Discrete(K)
    buf = GraphReplayBuffer(args, A, sp((D,)), sp((D,)), sp((E, 7)), sp((1,)), sp((1,)), sp((E, E)), space)
    if dt == torch.float64:                                 # the truth keeps its precision between the steps
        for k, v in list(vars(buf).items()):
            if isinstance(v, np.ndarray) and v.dtype == np.float32:
                setattr(buf, k, v.astype(np.float64))
    trainer = types.SimpleNamespace(prep_rollout=lambda: None, policy=pol, value_normalizer=vn)
    runner = types.SimpleNamespace(n_rollout_threads=N, num_agents=A, recurrent_N=1, hidden_size=64, use_centralized_V=False, buffer=buf,
                                   trainer=trainer, all_args=args, envs=types.SimpleNamespace(action_space=[space]))
    assert type(space).__name__ == "Discrete"
    buf.share_obs[0], buf.obs[0], buf.node_obs[0], buf.adj[0] = env["obs"][0], env["obs"][0], env["node_obs"][0], env["adj"][0]
    buf.agent_id[0], buf.share_agent_id[0] = env["agent_id"][0], env["agent_id"][0]
    out = {k: [] for k in ("values", "actions", "action_log_probs")}
    finished = None
    active_masks = np.ones((N, A, 1), np.int32)
    for step in range(T):
        if step == 0:
            values, actions, lp, h, hc, _ = GMPERunner.collect(runner, step)
            available = np.ones((N, A, K), np.float32)
        else:
            values, actions, lp, h, hc, _, available = GMPERunner.collect_with_mask(runner, step, None, active_masks, finished)
        dones = env["dones"][step]
        finished, _ = GMPERunner.get_finished(runner, dones)
        data = (env["obs"][step + 1], env["agent_id"][step + 1], env["node_obs"][step + 1], env["adj"][step + 1], env["agent_id"][step + 1],
                env["rewards"][step], dones, [{}] * N, values, actions, lp, h, hc, available)
        GMPERunner.insert(runner, data)
        for k, v in zip(("values", "actions", "action_log_probs"), (values, actions, lp)):
            out[k].append(np.array(v))
    GMPERunner.compute(runner)
    res = {k: np.array(v) for k, v in out.items()}
    for k in ("rnn_states", "rnn_states_critic", "value_preds", "returns", "masks", "active_masks", "available_actions"):
        res[k] = np.array(getattr(buf, k))
    return res, init, norm, margin[0], logits


def case_fixture(REF, case, seed, S):
    env = draw_env(seed, S)
    runs = {}
    for dt in (torch.float64, torch.float32):
        res, init, norm, margin, logits = run(REF, case, dt, seed, env, S)
        if dt == torch.float64:
            MT.need(margin >= MT.MARGIN, "a ReLU pre-activation of %.3g" % margin)
            assert len(logits) == T
            for t, lg in enumerate(logits):
                av = torch.from_numpy(res["available_actions"][t + 1].reshape(N * A, -1))            # what step t acted with lies in slot t + 1
                top = lg.masked_fill(av == 0, -np.inf).sort(1).values
                MT.need(float((top[:, -1] - top[:, -2]).min()) >= MT.GAP, "step %d: two logits of a row within %.3g" % (t, MT.GAP))
        runs[dt] = res
    t64, r32 = runs[torch.float64], runs[torch.float32]
    rec = dict(args=np.array(json.dumps(dict(RL.RETURNS_ARGS, use_popart=case == "popart", use_valuenorm=case == "valuenorm"))), seed=np.int64(seed))
    table = []
    for k in RL.EXACT:
        assert np.array_equal(t64[k], r32[k]), k
        rec["truth:" + k] = t64[k].astype(np.int64 if k == "actions" else np.float32)
    for k in RL.CLOSE:
        e = TL.err(r32[k], t64[k])
        MT.need(e <= TL.CAP, "%s err_ref %.3g" % (k, e))
        rec["truth:" + k], rec["err_ref:" + k] = t64[k].astype(np.float64), np.float64(e)
        table.append((case, k, e))
    dn = env["dones"]
    assert (t64["rnn_states"][1:][dn] == 0).all() and (np.abs(t64["rnn_states"][1:][~dn]).max(axis=(-1, -2)) > 0).all()
    assert (t64["actions"][1:][dn[:-1]] == S["K"] // 2).all() and (t64["available_actions"][2:][dn[:-1]].sum(-1) == 1).all()
    rec.update({"env:" + k: v for k, v in env.items()})
    rec.update({"init:%s:%s" % (net, k): v for net, sd in init.items() for k, v in sd.items()})
    rec.update({"norm:" + k: v for k, v in norm.items()})
    print("%s: seed %d, smallest |pre-activation| %.3g" % (case, seed, margin))
    return rec, table


def main():
    torch.set_num_threads(1)
    REF = MT.load_reference()
    S = RL.shapes()
    print("shapes", S)
    table, sizes = [], {}
    for case in RL.CASES:
        seed, (rec, rows) = MT.first_seed(lambda s: case_fixture(REF, case, s, S), case)
        table += rows
        sizes["rollout_%s.npz" % case] = MT.write("rollout_%s.npz" % case, rec)
    print("%-12s %-20s %s" % ("case", "array", "err_ref"))
    for case, what, e in table:
        print("%-12s %-20s %.3g" % (case, what, e))
    for k in sorted(sizes):
        print("  %-24s %d" % (k, sizes[k]))


if __name__ == "__main__":
    main()
