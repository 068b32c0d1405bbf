"""gmpe.policy over the table form: the generators' adj="table" against the same draw with adj="matrix", one ppo_update from each form, and collect_step /
compute on a buffer that keeps only entity tables against a buffer that keeps rows. The table form adds no arithmetic of its own and its GNNBase has
gnn_base's bits, so everything is compared with torch.equal: no tolerance anywhere.
N = 4 envs of A = 3 agents (rot_inv family: F = 7, the shipped actor and critic GNNBase, 'node' and global mean), T = 6 steps of envs whose time limit is 4:
an auto-reset lies inside every window."""
import copy
import types

import pytest
import torch

import gmpe
import gnn_lib as G
from gmpe import policy
from gmpe.minibatch import TableRows
from test_gpu_collect import _PopArt, _ValueNorm
from test_gpu_parity import ROT
from test_gpu_policy import DEV, K, _Net
from test_gpu_ppo_update import _Critic, update_args

pytestmark = pytest.mark.gpu
N, A, T, LIMIT = 4, 3, 6, 4
STORED = ("obs", "agent_id", "rewards", "dones", "masks", "active_masks", "value_preds", "available_actions", "actions", "action_log_probs", "rnn_states",
          "rnn_states_critic", "returns")


def setup(norm, **engine_kw):
    """one engine with a warmed-up buffer, the shipped actor and critic, the value normaliser, the args"""
    from gmpe.engine import GmpeEngine
    from gmpe.rollout import DeviceRolloutBuffer
    cfg = gmpe.make_config(scenario_name=ROT, num_envs=N, num_agents=A, episode_length=LIMIT, seed=11)
    eng = GmpeEngine(cfg, device=0, **engine_kw)
    assert int(cfg.node_feats) == 7 and int(cfg.n_actions) == K and cfg.num_entities == 6
    actor = _Net(G.ACTOR, eng.D, "act").to(DEV)
    critic = _Critic(G.CRITIC, eng.D, "popart" if norm == "popart" else "v_out", seed=12).to(DEV)
    vn = None
    if norm == "popart":
        vn = critic.v_out = _PopArt(DEV)
        vn.mean.fill_(0.3), vn.mean_sq.fill_(0.7), vn.debiasing_term.fill_(0.5)
    else:
        vn = _ValueNorm(DEV)
        vn.running_mean.fill_(0.3), vn.running_mean_sq.fill_(0.7), vn.debiasing_term.fill_(0.5)
    args = update_args(use_popart=norm == "popart", use_valuenorm=norm == "valuenorm")
    for k, v in dict(gamma=0.99, gae_lambda=0.95, use_gae=True, use_proper_time_limits=False).items():
        setattr(args, k, v)
    buf = DeviceRolloutBuffer(eng, T, use_centralized_V=False, policy_fields="all", learner_fields="all", args=args, recurrent_N=1, hidden_size=64)
    buf.warmup()
    return cfg, eng, buf, actor, critic, vn, args


def filled(norm):
    """a buffer that keeps rows, a compact adjacency and tables, filled by one rollout of the policy"""
    cfg, eng, buf, actor, critic, vn, args = setup(norm, node_form="both", adj_compact=True)
    policy.rollout(actor, critic, buf, vn)
    dn = buf.dones.bool()
    assert bool(dn.any()) and not bool(dn.all())        # the time limit lies inside the window
    return cfg, eng, buf, actor, critic, vn, args


def samples(buf, adv, recurrent, adj):
    """the minibatches of one epoch with a fixed permutation; remainders: 72 samples in 5 minibatches of 14, 24 chunks of 3 in 5 minibatches of 4"""
    if recurrent:
        perm = torch.randperm(T * N * A // 3, generator=torch.Generator().manual_seed(5))
        return list(buf.recurrent_generator(adv, 5, 3, perm=perm, adj=adj))
    perm = torch.randperm(T * N * A, generator=torch.Generator().manual_seed(4))
    return list(buf.feed_forward_generator(adv, 5, perm=perm, adj=adj))


@pytest.mark.parametrize("recurrent", [False, True], ids=["feed_forward", "recurrent"])
def test_adj_table_yields_the_matrix_draws_other_entries_and_the_same_graphs(recurrent):
    cfg, eng, buf, actor, critic, vn, args = filled("valuenorm")
    adv = buf.normalized_advantages(vn)
    ms, ts = samples(buf, adv, recurrent, "matrix"), samples(buf, adv, recurrent, "table")
    assert len(ms) == len(ts) == 5
    for m, t in zip(ms, ts):
        assert len(m) == len(t) == 16 and t[2] is None and isinstance(t[3], TableRows)
        for i in range(16):
            if i not in (2, 3):
                assert (m[i] is None and t[i] is None) or torch.equal(m[i], t[i]), i
        rows = m[2].shape[0]
        assert rows == (12 if recurrent else 14)
        tr = t[3]
        assert tr.table.data_ptr() == buf.entity_table.data_ptr() and tr.table.shape == buf.entity_table.shape and tr.cfg is cfg       # not copied
        assert tr.index.dtype == torch.int64 and tuple(tr.index.shape) == (rows,) and 0 <= int(tr.index.min()) and int(tr.index.max()) < T * N
        with torch.no_grad():
            for net, ids in ((actor, t[4]), (critic, t[5])):
                got = gmpe.gnn_base_from_table(tr.table, tr.index, ids, net.gnn_base, cfg)
                assert torch.equal(got, gmpe.gnn_base(m[2], m[3], ids, net.gnn_base))
    eng.check_errors()


def state_of(actor, critic, aopt, copt, vn):
    out = {"actor." + k: p for k, p in actor.named_parameters()}
    out.update({"critic." + k: p for k, p in critic.named_parameters()})
    for k in ("running_mean", "running_mean_sq", "debiasing_term", "weight", "bias", "stddev", "mean", "mean_sq"):
        if isinstance(getattr(vn, k, None), torch.Tensor):
            out["norm." + k] = getattr(vn, k)
    for tag, opt in (("aopt", aopt), ("copt", copt)):
        for i, p in enumerate(q for g in opt.param_groups for q in g["params"]):
            for k, v in opt.state.get(p, {}).items():
                out["%s.%d.%s" % (tag, i, k)] = torch.as_tensor(v)
    return {k: v.detach().clone() for k, v in out.items()}


@pytest.mark.parametrize("norm", ["valuenorm", "popart"])
@pytest.mark.parametrize("recurrent", [False, True], ids=["feed_forward", "recurrent"])
def test_one_ppo_update_from_each_form_leaves_equal_parameters_moments_and_normaliser(recurrent, norm):
    cfg, eng, buf, actor, critic, vn, args = filled(norm)
    adv = buf.normalized_advantages(vn)
    results = []
    for adj in ("matrix", "table"):
        a, c = copy.deepcopy(actor), copy.deepcopy(critic)
        v = c.v_out if norm == "popart" else copy.deepcopy(vn)
        aopt, copt = (torch.optim.Adam(list(n.parameters()), lr=5e-4, eps=1e-5, weight_decay=0) for n in (a, c))
        before = state_of(a, c, aopt, copt, v)
        s = samples(buf, adv, recurrent, adj)[1]
        u = policy.ppo_update(a, c, aopt, copt, s, args, v)
        torch.cuda.synchronize()
        after = state_of(a, c, aopt, copt, v)
        assert any(k.startswith("actor.") and not torch.equal(before[k], after[k]) for k in before)
        assert any(k.startswith("norm.") and not torch.equal(before[k], after[k]) for k in before)
        results.append((u, after))
    (um, am), (ut, at) = results
    assert sorted(am) == sorted(at) and any(".exp_avg" in k for k in am)
    for k in am:
        assert torch.equal(am[k], at[k]), k
    for k in um._fields:
        assert torch.equal(getattr(um, k), getattr(ut, k)), k
    eng.check_errors()


def test_train_with_graph_table_is_train_with_rows():
    cfg, eng, buf, actor, critic, vn, args = filled("valuenorm")
    args.ppo_epoch, args.num_mini_batch, args.data_chunk_length, args.use_recurrent_policy = 2, 2, 3, True
    perms = [torch.randperm(T * N * A // 3, generator=torch.Generator().manual_seed(s)) for s in (1, 2)]
    outs = []
    for graph in ("rows", "table"):
        a, c, v = copy.deepcopy(actor), copy.deepcopy(critic), copy.deepcopy(vn)
        aopt, copt = (torch.optim.Adam(list(n.parameters()), lr=5e-4, eps=1e-5, weight_decay=0) for n in (a, c))
        info = policy.train(a, c, aopt, copt, buf, args, v, perms=perms, graph=graph)
        outs.append((info, state_of(a, c, aopt, copt, v)))
    (im, sm), (it, st) = outs
    for k in im:
        assert torch.equal(im[k], it[k]) and bool(torch.isfinite(im[k])), k
    for k in sm:
        assert torch.equal(sm[k], st[k]), k
    with pytest.raises(NotImplementedError, match="TableRows"):
        policy.CapturedUpdate(actor, critic, aopt, copt, samples(buf, buf.advantages, True, "table")[0], args, vn)
    eng.check_errors()


def test_collect_steps_and_compute_on_a_table_only_buffer_store_what_a_rows_buffer_stores():
    _, er, br, actor, critic, vn, _ = setup("valuenorm")
    cfg, et, bt, _, _, _, _ = setup("valuenorm", node_form="table", adj_form="none")
    assert bt._node_obs is None and bt._adj is None and bt.entity_table is not None and br.entity_table is None
    for b in (br, bt):
        for _ in range(T):
            policy.collect_step(actor, critic, b)
        returns = policy.compute(critic, b, copy.deepcopy(vn))
        assert returns is b.returns and b.step == 0     # the window is full: the next step is an after_update away
    torch.cuda.synchronize()
    dn = br.dones.bool()
    assert bool(dn.any()) and not bool(dn.all())        # an auto-reset inside the window
    for k in STORED:
        x, y = getattr(br, k), getattr(bt, k)
        assert x is not None and y is not None and x.dtype == y.dtype and torch.equal(x, y), k
    assert torch.equal(bt.node_obs, br._node_obs) and torch.equal(bt.adj, br.adj)
    assert float(br.value_preds.abs().max()) > 0 and bool(torch.isfinite(br.returns).all())
    # rollout() takes the same buffer from step 0
    bt.after_update(), br.after_update()
    assert torch.equal(policy.rollout(actor, critic, bt, copy.deepcopy(vn)), policy.rollout(actor, critic, br, copy.deepcopy(vn)))
    for e in (er, et):
        e.check_errors()
