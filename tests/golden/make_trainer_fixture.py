"""Golden vectors for the composed learner (gmpe.policy.ppo_update / train / actor_forward / critic_forward), produced by RUNNING the reference's
trainer on the CPU, in the build container only:

    python tests/golden/make_trainer_fixture.py        # writes tests/golden/trainer_*.npz and prints the err_ref table

What runs is the reference's own code, imported through ref_harness with the stubs of make_ppo_loss_fixture.py / make_buffer_fixture.py: GR_Actor and
GR_Critic (graph_actor_critic.py) with their MLPBase, RNNLayer, ACTLayer and PopArt, GR_MAPPO.ppo_update and GR_MAPPO.train (graph_mappo.py) with its
ValueNorm, clip_grad_norm_ and torch.optim.Adam(lr=5e-4, eps=1e-5, weight_decay=0), and GraphReplayBuffer filled through GMPERunner.insert. The policy
object is a namespace with the four attributes GR_MAPPO reads and an evaluate_actions that calls actor.evaluate_actions and critic.forward, as
graph_MAPPOPolicy.py does.

THE ONE SWAP: onpolicy/algorithms/utils/gnn_new.py needs torch_geometric, which is absent, so that one module is replaced by an adapter around
tests/gnn_lib.py's restatement (ConvNet + forward), which tests/test_gpu_gnn.py already pins the kernels to. Nothing else is restated.

Weights: the shipped GNNBase and head weights (gnn_base.npz, policy_heads.npz); the reference's seeded init for the MLPBase and the RNNLayer.
Every run is executed twice: float32 as shipped, and float64 (modules .double(), every tpdv["dtype"] of actor, critic, trainer, PopArt and ValueNorm
set to float64). The float64 run is the truth, the float32 run only supplies err_ref = max|a32 - a64| / max|a64|. Asserted here, for every stored
array and scalar: err_ref <= 1e-5; |truth| >= 1e-2 for every scalar (the actor's norm without update_actor is exactly 0 and stored as such); both norms
above max_grad_norm where the clip is on; every pre-activation in front of a ReLU at least 1e-5 from zero in the float64 run (a flip
between two float32 computations is an error of the inputs, not of either computation); in the forward record,
every row's top two logits at least 1e-4 apart. A seed that fails is replaced by the next. Data only is written."""
import argparse
import io
import json
import os
import sys
import types
import warnings
import zipfile

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
import trainer_lib as TL  # noqa: E402

MARGIN, GAP = 1e-5, 1e-4                                # gnn_lib's and mlp_lib's margin
N_ENVS, AGENTS, T = 2, 3, 8                             # the train buffer: 48 rows, 24 per minibatch (six chunks of four)


class GNNBase(nn.Module):
    """the adapter: gnn_new.GNNBase's constructor and forward signature around gnn_lib, with the shipped weights"""

    def __init__(self, args, node_obs_shape, edge_dim, aggr):
        super().__init__()
        assert node_obs_shape == 7 and edge_dim == 1
        self.gnn = G.build(G.config("actor" if aggr == "node" else "critic")).gnn
        self.out_dim = G.C

    def forward(self, node_obs, adj, agent_id):
        return G.forward(self, node_obs, adj, agent_id.reshape(-1))


def load_reference():
    MB.load_reference()
    MB._stub("onpolicy.algorithms.utils.gnn_new", GNNBase=GNNBase)
    MB._stub("onpolicy.algorithms.graph_MAPPOPolicy", GR_MAPPOPolicy=object)
    from onpolicy.algorithms.graph_actor_critic import GR_Actor, GR_Critic
    from onpolicy.algorithms.graph_mappo import GR_MAPPO
    return GR_Actor, GR_Critic, GR_MAPPO


def ref_args(a):
    return argparse.Namespace(hidden_size=64, gain=0.01, use_orthogonal=True, recurrent_N=1, actor_graph_aggr="node", critic_graph_aggr="global",
                              use_feature_normalization=True, use_ReLU=True, stacked_frames=1, layer_N=1, use_cent_obs=True, num_agents=AGENTS, **vars(a))


def build(REF, a, dt, seed):
    """the reference's actor, critic, policy namespace and trainer in dtype dt; the smallest |pre-activation| any ReLU saw lands in trainer.margin"""
    import gym
    GR_Actor, GR_Critic, GR_MAPPO = REF
    sp = lambda s: gym.spaces.Box(-np.inf, np.inf, s, np.float32)
    args = ref_args(a)
    torch.manual_seed(seed)
    actor = GR_Actor(args, sp((TL.OBS,)), sp((TL.E, 7)), sp((1,)), gym.spaces.Discrete(TL.K))
    critic = GR_Critic(args, sp((TL.OBS,)), sp((TL.E, 7)), sp((1,)))
    g = HL.golden()
    with torch.no_grad():
        actor.act.action_out.linear.weight.copy_(torch.from_numpy(g["actor.act.action_out.linear.weight"]))
        actor.act.action_out.linear.bias.copy_(torch.from_numpy(g["actor.act.action_out.linear.bias"]))
        critic.v_out.weight.copy_(torch.from_numpy(g["critic.v_out.weight"]))
        critic.v_out.bias.copy_(torch.from_numpy(g["critic.v_out.bias"]))
        if a.use_popart:
            critic.v_out.stddev.copy_(torch.from_numpy(g["critic.v_out.stddev"]))
    actor, critic = actor.to(dt), critic.to(dt)
    actor.tpdv["dtype"] = critic.tpdv["dtype"] = dt
    if a.use_popart:
        critic.v_out.tpdv["dtype"] = dt
    adam = lambda net: torch.optim.Adam(net.parameters(), lr=TL.LR, eps=TL.EPS, weight_decay=0)
    pol = types.SimpleNamespace(actor=actor, critic=critic, actor_optimizer=adam(actor), critic_optimizer=adam(critic))

    def evaluate_actions(share_obs, obs, node_obs, adj, agent_id, share_agent_id, h, hc, action, masks, available_actions=None, active_masks=None):
        lp, ent = actor.evaluate_actions(obs, node_obs, adj, agent_id, h, action, masks, available_actions, active_masks)
        values, _ = critic(share_obs, node_obs, adj, share_agent_id, hc, masks)
        return values, lp, ent
    pol.evaluate_actions = evaluate_actions
    tr = GR_MAPPO(args, pol)
    tr.tpdv["dtype"] = dt
    tr.update_counter = 0
    if a.use_valuenorm:
        tr.value_normalizer.to(dt)
        tr.value_normalizer.tpdv["dtype"] = dt
    tr.margin = [np.inf]

    def seen(mod, inp):
        tr.margin[0] = min(tr.margin[0], float(inp[0].detach().abs().min())) if inp[0].numel() else tr.margin[0]
    for net in (actor, critic):
        for m in set(m for m in net.modules() if isinstance(m, nn.ReLU)):
            m.register_forward_pre_hook(seen)
    tr.born = {id(p): "%s.%s" % (tag, k) for tag, net in (("actor", actor), ("critic", critic)) for k, p in net.named_parameters()}
    return pol, tr


def draw_sample(seed):
    """one 30-row sample (6 steps x 5 rows, E = 7, obs 6, K = 25) as the generators' 16-tuple of numpy arrays"""
    rng = np.random.RandomState(9000 + seed)
    f32, R = np.float32, TL.ROWS
    x, adj, ids = G.draw(rng, R, TL.E, 7)
    av = (rng.rand(R, TL.K) > 0.3).astype(f32)
    av[:, TL.K // 2] = 1
    actions = np.array([rng.choice(np.flatnonzero(r)) for r in av], f32).reshape(R, 1)
    u = lambda: rng.uniform(-1, 1, (TL.NB, 1, 64)).astype(f32)
    return (rng.randn(R, TL.OBS).astype(f32), rng.randn(R, TL.OBS).astype(f32), x, adj, ids.reshape(R, 1), ids.reshape(R, 1).copy(), u(), u(), actions,
            rng.randn(R, 1).astype(f32), rng.randn(R, 1).astype(f32), (rng.rand(R, 1) > 0.2).astype(f32), (rng.rand(R, 1) > 0.1).astype(f32),
            (-rng.rand(R, 1) * 3).astype(f32), rng.randn(R, 1).astype(f32), av)


def final(pol, tr):
    return {"actor": TL.collect(pol.actor, pol.actor_optimizer, tr.born), "critic": TL.collect(pol.critic, pol.critic_optimizer, tr.born)}


def state_dict(net):
    return {k: v.detach().float().numpy().copy() for k, v in net.state_dict().items()}


class Refused(Exception):
    pass


def need(cond, what):
    if not cond:
        raise Refused(what)


def summarise(rec, runs, stored, scalars_names, table, case):
    """the truth, the err_ref and the asserts of one case from its float64 and float32 runs; runs[dt] = (scalars, collected, imp or None)"""
    (s64, c64, i64), (s32, c32, i32) = runs[torch.float64], runs[torch.float32]
    rec["scalars"] = s64
    e = np.zeros(s64.shape)
    for i in np.ndindex(*s64.shape):
        if s64[i] == 0.0:
            need(s32[i] == 0.0, "a scalar that is exactly 0 in float64 only")
            continue
        e[i] = TL.err(s32[i], s64[i])
        need(abs(s64[i]) >= 1e-2, "%s is %.3g: under 1e-2 in magnitude" % (scalars_names[i[-1]], s64[i]))
        need(e[i] <= TL.CAP, "%s err_ref %.3g" % (scalars_names[i[-1]], e[i]))
    rec["scalars:err_ref"] = e
    table.append((case, "scalars (worst)", float(e.max())))
    if i64 is not None:
        rec["imp_weights"], rec["imp_weights:err_ref"] = i64, TL.err(i32, i64)
        need(rec["imp_weights:err_ref"] <= TL.CAP, "imp_weights err_ref %.3g" % rec["imp_weights:err_ref"])
        table.append((case, "imp_weights", rec["imp_weights:err_ref"]))
    arrays = {}
    for net in stored:
        names = list(c64[net])
        assert names == list(c32[net])
        meta = dict(names=names, sizes=[c64[net][n]["param"].size for n in names], has_grad=[c64[net][n]["grad"] is not None for n in names],
                    steps=[c64[net][n]["step"] for n in names])
        assert meta["steps"] == [c32[net][n]["step"] for n in names] and meta["has_grad"] == [c32[net][n]["grad"] is not None for n in names]
        a64, a32 = TL.arrays_of(c64[net], meta), TL.arrays_of(c32[net], meta)
        rec["%s:names" % net], rec["%s:sizes" % net] = np.array(names), np.array(meta["sizes"], np.int64)
        rec["%s:has_grad" % net], rec["%s:steps" % net] = np.array(meta["has_grad"]), np.array(meta["steps"], np.int64)
        for kind in TL.KINDS:
            er = TL.err(a32[kind], a64[kind])
            need(er <= TL.CAP, "%s %s err_ref %.3g" % (net, kind, er))
            rec["%s:err_ref:%s" % (net, kind)] = er
            table.append((case, "%s %s" % (net, kind), er))
        arrays[net] = a64
    rec["stored"] = np.array(json.dumps(list(stored)))
    return arrays


def update_case(REF, case, samples, seed):
    a = TL.case_args(case)
    runs, table = {}, []
    for dt in (torch.float64, torch.float32):
        pol, tr = build(REF, a, dt, seed)
        init = None if dt != torch.float32 else {"actor": state_dict(pol.actor), "critic": state_dict(pol.critic)}
        scalars, imps = [], []
        for s in samples:
            out = tr.ppo_update(s, TL.CASES[case][1])
            scalars.append([float(out[i]) for i in range(5)] + [float(out[5].mean())])
            imps.append(out[5].detach().double().numpy())
            if a.use_max_grad_norm:
                need(float(out[1]) > a.max_grad_norm and (not TL.CASES[case][1] or float(out[4]) > a.max_grad_norm), "the clip does not bite")
        need(dt != torch.float64 or tr.margin[0] >= MARGIN, "a ReLU pre-activation of %.3g" % tr.margin[0])
        margin = tr.margin[0] if dt == torch.float64 else margin
        runs[dt] = (np.array(scalars), final(pol, tr), np.array(imps))
    rec = dict(args=np.array(json.dumps(vars(a))))
    arrays = summarise(rec, runs, TL.CASES[case][2], TL.SCALARS, table, case)
    print("%s: seed %d, smallest |pre-activation| %.3g" % (case, seed, margin))
    return rec, arrays, init, table


def fill_buffer(seed):
    """the reference's GraphReplayBuffer, filled through GMPERunner.insert as make_buffer_fixture.py fills one, with graphs as gnn_lib draws them"""
    GraphReplayBuffer, GMPERunner = MB.load_reference()
    import gym
    Box, Discrete = gym.spaces.Box, gym.spaces.Discrete
    N, A, E, D = N_ENVS, AGENTS, TL.E, TL.OBS
    args = argparse.Namespace(episode_length=T, n_rollout_threads=N, hidden_size=64, recurrent_N=1, gamma=0.99, gae_lambda=0.95, use_gae=True,
                              use_popart=False, use_valuenorm=False, use_proper_time_limits=False, use_centralized_V=False)
    sp = lambda shape: Box(-np.inf, np.inf, shape, np.float32)
    buf = GraphReplayBuffer(args, A, sp((D,)), sp((D,)), sp((E, 7)), sp((1,)), sp((1,)), sp((E, E)), Discrete(TL.K))
    runner = types.SimpleNamespace(n_rollout_threads=N, num_agents=A, recurrent_N=1, hidden_size=64, use_centralized_V=False, buffer=buf)
    rng = np.random.RandomState(seed)
    f32 = np.float32

    def step():
        x, adj, ids = G.draw(rng, N * A, E, 7)
        return rng.randn(N, A, D), x.reshape(N, A, E, 7), adj.reshape(N, A, E, E), ids.reshape(N, A, 1)
    obs, x, adj, ids = step()
    buf.share_obs[0], buf.obs[0], buf.node_obs[0], buf.adj[0], buf.agent_id[0], buf.share_agent_id[0] = obs, obs, x, adj, ids, ids
    for t in range(T):
        obs, x, adj, ids = step()
        dones = rng.rand(N, A) < 0.25
        av = (rng.rand(N, A, TL.K) > 0.3).astype(f32)
        av[:, :, TL.K // 2] = 1
        actions = np.array([rng.choice(np.flatnonzero(r)) for r in buf.available_actions[t].reshape(N * A, TL.K)], f32).reshape(N, A, 1)
        data = (obs, ids, x, adj, ids, rng.randn(N, A, 1), dones, [{}] * N, rng.randn(N, A, 1).astype(f32), actions,
                (-rng.rand(N, A, 1) * 3).astype(f32), rng.uniform(-1, 1, (N, A, 1, 64)).astype(f32), rng.uniform(-1, 1, (N, A, 1, 64)).astype(f32), av)
        GMPERunner.insert(runner, data)
    buf.compute_returns(rng.randn(N, A, 1).astype(f32), None)
    return buf


def train_case(REF, case, seed):
    a = TL.case_args(case)
    runs, calls, yielded, adv, table = {}, None, None, None, []
    for dt in (torch.float64, torch.float32):
        pol, tr = build(REF, a, dt, seed)
        init = {"actor": state_dict(pol.actor), "critic": state_dict(pol.critic)}
        buf = fill_buffer(500 + seed)
        log, out, advs = [], [], []
        for method in ("recurrent_generator", "feed_forward_generator", "naive_recurrent_generator"):
            def wrapped(advantages, *args, _m=method, _f=getattr(buf, method)):
                assert len(args) == (2 if _m == "recurrent_generator" else 1)
                advs.append(np.array(advantages))
                entry = [_m, int(args[0]), int(args[1]) if len(args) > 1 else None, 0]
                log.append(entry)
                for s in _f(advantages, *args):
                    entry[3] += 1
                    out.append(tuple(np.array(v) for v in s))
                    yield s
            setattr(buf, method, wrapped)
        torch.manual_seed(77 + seed)
        info = tr.train(buf)
        need(dt != torch.float64 or tr.margin[0] >= MARGIN, "a ReLU pre-activation of %.3g" % tr.margin[0])
        runs[dt] = (np.array([float(info[k]) for k in TL.TRAIN_INFO]), final(pol, tr), None)
        if calls is not None:                           # the float32 run drew the same samples
            assert calls == log and all(np.array_equal(p, q) for s, t in zip(yielded, out) for p, q in zip(s, t))
        calls, yielded, adv = log, out, advs
    assert all(np.array_equal(adv[0], x) for x in adv) and len(calls) == a.ppo_epoch
    rec = dict(args=np.array(json.dumps(vars(a))), calls=np.array(json.dumps(calls)), advantages=adv[0])
    for i, s in enumerate(yielded):
        rec.update({"yield%d:%s" % (i, k): v for k, v in zip(TL.SAMPLE, s)})
    arrays = summarise(rec, runs, ("actor", "critic"), TL.TRAIN_INFO, table, case)
    return rec, arrays, init, table


def forward_record(REF, sample, seed):
    a = TL.case_args("plain")
    rec, runs = {}, {}
    for dt in (torch.float64, torch.float32):
        pol, tr = build(REF, a, dt, seed)
        logits = []
        pol.actor.act.action_out.linear.register_forward_hook(lambda m, i, o: logits.append(o.detach().clone()))
        share_obs, obs, x, adj, ids, sids, h, hc = sample[:8]
        with torch.no_grad():
            actions, lp, ho = pol.actor(obs, x, adj, ids, h, sample[11], sample[15], deterministic=True)
            values, hco = pol.critic(share_obs, x, adj, sids, hc, sample[11])
        if dt == torch.float64:
            top = logits[0].masked_fill(torch.from_numpy(sample[15]) == 0, -np.inf).sort(1).values
            need(float((top[:, -1] - top[:, -2]).min()) >= GAP, "two logits of a row within %.3g" % GAP)
            need(tr.margin[0] >= MARGIN, "a ReLU pre-activation of %.3g" % tr.margin[0])
        runs[dt] = dict(actions=actions, action_log_probs=lp, rnn_states=ho, values=values, rnn_states_critic=hco)
    t, r = runs[torch.float64], runs[torch.float32]
    assert torch.equal(t["actions"], r["actions"])
    rec["forward:actions"] = t["actions"].numpy()
    for k in ("action_log_probs", "rnn_states", "values", "rnn_states_critic"):
        rec["forward:" + k] = t[k].double().numpy()
        rec["forward:err_ref:" + k] = TL.err(r[k].double().numpy(), rec["forward:" + k])
        assert rec["forward:err_ref:" + k] <= TL.CAP, k
    return rec


def write(name, rec):
    """an .npz whose bytes depend on its contents alone: sorted names, a fixed date, deflate"""
    p = os.path.join(HERE, name)
    with zipfile.ZipFile(p, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(rec):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asanyarray(rec[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type, info.external_attr = zipfile.ZIP_DEFLATED, 0o644 << 16
            z.writestr(info, b.getvalue())
    size = os.path.getsize(p)
    assert size <= TL.MAX_FILE, (name, size)
    return size


def first_seed(fn, what, start=5):
    for seed in range(start, start + 40):
        try:
            return seed, fn(seed)
        except Refused as e:
            print("%s: seed %d refused: %s" % (what, seed, e))
    raise SystemExit("%s: none of 40 seeds meets the conditions" % what)


def main():
    torch.set_num_threads(1)
    REF = load_reference()
    table, sizes, inputs = [], {}, {}

    def all_updates(seed):
        samples = [draw_sample(10 * seed + i) for i in range(TL.UPDATES)]
        out = {case: update_case(REF, case, samples, seed) for case in TL.CASES}
        return samples, out, forward_record(REF, samples[0], seed)
    seed, (samples, out, fwd) = first_seed(all_updates, "ppo_update")
    for i, s in enumerate(samples):
        inputs.update({"sample%d:%s" % (i, k): v for k, v in zip(TL.SAMPLE, s)})
    inputs["seed"] = np.int64(seed)
    inputs.update(fwd)
    for case, (rec, arrays, init, rows) in out.items():
        table += rows
        tag = case.replace("-", "_")
        if case in ("plain", "popart"):
            for net, sd in init.items():
                if case == "plain" or net == "critic":
                    inputs.update({"init:%s:%s" % (net if case == "plain" else "critic_popart", k): v for k, v in sd.items()})
        sizes["trainer_%s.npz" % tag] = write("trainer_%s.npz" % tag, rec)
        for net, a in arrays.items():
            for half, kinds in (("gp", ("grad", "param")), ("mv", ("exp_avg", "exp_avg_sq"))):
                name = "trainer_%s_%s_%s.npz" % (tag, net, half)
                sizes[name] = write(name, {k: a[k] for k in kinds})
    for case in TL.TRAIN_CASES:
        tseed, (rec, arrays, init, rows) = first_seed(lambda s: train_case(REF, case, s), case, seed)
        rec["seed"] = np.int64(tseed)
        if tseed != seed:                               # else the networks start from trainer_inputs.npz's initial state
            rec.update({"init:%s:%s" % (net, k): v for net, sd in init.items() for k, v in sd.items()})
        table += rows
        tag = case.replace("-", "_")
        sizes["trainer_%s.npz" % tag] = write("trainer_%s.npz" % tag, rec)
        for net, a in arrays.items():
            for half, kinds in (("gp", ("grad", "param")), ("mv", ("exp_avg", "exp_avg_sq"))):
                name = "trainer_%s_%s_%s.npz" % (tag, net, half)
                sizes[name] = write(name, {k: a[k] for k in kinds})
    sizes["trainer_inputs.npz"] = write("trainer_inputs.npz", inputs)
    print("%-20s %-28s %s" % ("case", "array", "err_ref"))
    for case, what, e in table:
        print("%-20s %-28s %.3g" % (case, what, e))
    for k in ("action_log_probs", "rnn_states", "values", "rnn_states_critic"):
        print("%-20s %-28s %.3g" % ("forward", k, float(fwd["forward:err_ref:" + k])))
    print("files: %d, %d bytes in all, the largest %d" % (len(sizes), sum(sizes.values()), max(sizes.values())))
    for k in sorted(sizes):
        print("  %-44s %d" % (k, sizes[k]))


if __name__ == "__main__":
    main()
