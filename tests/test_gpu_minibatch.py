"""PPO minibatches gathered on the device (gmpe_minibatch_gather; DeviceRolloutBuffer.feed_forward_generator / recurrent_generator).

* golden parity: a DeviceRolloutBuffer filled with the inputs of tests/golden/minibatch_generators.npz yields, for the reference's permutation and for
  torch.manual_seed(seed) + perm=None, exactly the arrays the reference's own generators yielded (recurrent T % L != 0 included);
* storage forms on engine rollouts (episodes with resets and goal reaches): rows + materialised adjacency, rows + compact adjacency and entity table + no
  adjacency all yield the reference-shaped reshape-and-index of the materialised arrays, learner arrays and recurrent chunk heads included, with the generator
  enqueued right after collect on the same stream;
* E >= 64 in the table form."""
import os

import numpy as np
import pytest

import gmpe
from test_gpu_gather import JULY, _queue
from test_gpu_parity import ROTFAM

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "minibatch_generators.npz")
NAMES = ("share_obs", "obs", "node_obs", "adj", "agent_id", "share_agent_id", "rnn_states", "rnn_states_critic", "actions", "value_preds", "returns", "masks",
         "active_masks", "action_log_probs", "advantages", "available_actions")


def _golden_buffer(torch, g, case):
    from gmpe.engine import GmpeEngine
    from gmpe.rollout import DeviceRolloutBuffer
    T, N, A = int(g["T"]), int(g["N"]), int(g["A"])
    cfg = gmpe.make_config(num_envs=N, num_agents=A, episode_length=T)
    assert (cfg.obs_dim, cfg.num_entities, cfg.node_feats, cfg.n_actions) == (int(g["D"]), int(g["E"]), int(g["F"]), int(g["n_actions"]))
    avail = bool(g[case + "_avail"])
    eng = GmpeEngine(cfg)                                                 # rows form, materialised adjacency
    buf = DeviceRolloutBuffer(eng, T, use_centralized_V=bool(g[case + "_centralized"]),
                              policy_fields=("value_preds", "returns") + (("available_actions",) if avail else ()))
    dev = eng.device
    put = lambda dst, k: dst.copy_(torch.as_tensor(g["in_" + k]).to(dev))
    for k, dst in (("obs", buf.obs), ("node_obs", buf._node_obs), ("adj", buf._adj), ("agent_id", buf.agent_id), ("masks", buf.masks),
                   ("active_masks", buf.active_masks), ("value_preds", buf.value_preds), ("returns", buf.returns)):
        put(dst, k)
    if avail:
        put(buf.available_actions, "available_actions")
    learner = {k: torch.as_tensor(g["in_" + k]).to(dev) for k in ("rnn_states", "rnn_states_critic", "actions", "action_log_probs")}
    return buf, learner, torch.as_tensor(g["in_advantages"]).to(dev)


@pytest.mark.parametrize("case", ["ff_one", "ff_rem", "rec_l5", "rec_l10"])
def test_generators_equal_the_reference_yields(case):
    import torch
    g = np.load(GOLD)
    buf, learner, adv = _golden_buffer(torch, g, case)
    nmb, L = int(g[case + "_num_mini_batch"]), int(g[case + "_data_chunk_length"])
    rec = bool(g[case + "_recurrent"])
    make = (lambda **kw: buf.recurrent_generator(adv, nmb, L, learner=learner, **kw)) if rec else \
        (lambda **kw: buf.feed_forward_generator(adv, nmb, learner=learner, **kw))
    runs = [list(make(perm=torch.as_tensor(g[case + "_perm"])))]
    torch.manual_seed(int(g[case + "_seed"]))
    runs.append(list(make()))                                             # perm=None: the reference's draw on the CPU default generator
    for batches in runs:
        assert len(batches) == int(g[case + "_num_batches"])
        for b, tup in enumerate(batches):
            assert len(tup) == 16
            for k, v in zip(NAMES, tup):
                if bool(g["%s_%d_%s_none" % (case, b, k)]):
                    assert v is None, (case, b, k)
                    continue
                ref = torch.as_tensor(g["%s_%d_%s" % (case, b, k)])
                assert v.device == buf.engine.device and v.dtype == ref.dtype and torch.equal(v.cpu(), ref), (case, b, k)
    # perm="device": other draws, the same shapes and dtypes
    d = list(make(perm="device"))
    assert [[None if v is None else (v.shape, v.dtype) for v in t] for t in d] == [[None if v is None else (v.shape, v.dtype) for v in t] for t in runs[0]]
    with pytest.raises(NotImplementedError):
        buf.naive_recurrent_generator(adv, nmb)


def _reference_batches(torch, arrays, centralized, perm, sampler, L=None):
    """the reference's generators restated in torch on the materialised arrays (graph_buffer.py:401-465, 624-758), for comparison on the device"""
    T1, N, A, D = arrays["obs"].shape
    T = T1 - 1
    share_obs = arrays["obs"].reshape(T1, N, 1, A * D).expand(T1, N, A, A * D) if centralized else arrays["obs"]
    share_id = arrays["agent_id"].reshape(T1, N, 1, A).expand(T1, N, A, A) if centralized else arrays["agent_id"]
    src = dict(arrays, share_obs=share_obs, share_agent_id=share_id)
    out = []
    for off, rows in sampler:
        idx = perm[off:off + rows]
        o = {}
        for k in NAMES:
            x = src[k]
            x = x[:-1] if x.shape[0] == T1 else x
            if L is None:
                o[k] = x.reshape(-1, *x.shape[3:])[idx]
            else:
                y = x.permute(1, 2, 0, *range(3, x.dim())).reshape(-1, *x.shape[3:])
                if k.startswith("rnn"):
                    o[k] = torch.stack([y[int(c) * L] for c in idx])
                else:
                    o[k] = torch.stack([y[int(c) * L:int(c) * L + L] for c in idx], dim=1).reshape(L * rows, *x.shape[3:])
        out.append(o)
    return out


def _rollout_buffers(torch, scen, feat, N, A, T, seed):
    from gmpe.engine import GmpeEngine
    from gmpe.rollout import DeviceRolloutBuffer
    nav = scen == "navigation_graph"
    kw = dict(scenario_name=scen, num_envs=N, num_agents=A, world_size=2.4, episode_length=6, seed=seed, graph_feat_type=feat)
    if nav:
        kw.update(num_obstacles=2, num_landmarks=5)
    cfg = gmpe.make_config(**kw)
    engines = [GmpeEngine(cfg), GmpeEngine(cfg, adj_compact=True), GmpeEngine(cfg, adj_compact=True, node_form="table", adj_form="none")]
    bufs = [DeviceRolloutBuffer(e, T, policy_fields="all") for e in engines]
    for b in bufs:
        b.warmup()
    if not nav:
        _queue(engines[0], engines, np.random.RandomState(4), N, A)      # goal reaches within the rollout
    return cfg, bufs


@pytest.mark.parametrize("feat", ["relative", "global"])
@pytest.mark.parametrize("scen", [JULY, "navigation_graph"] + ROTFAM)
def test_storage_forms_yield_the_reference_indexing_of_engine_rollouts(scen, feat):
    import torch
    from gmpe.minibatch import feed_forward_sizes, recurrent_sizes
    N, A, T, L = 13, 4, 9, 4                                              # T % L != 0: chunks cross agent and env boundaries
    cfg, bufs = _rollout_buffers(torch, scen, feat, N, A, T, 31)
    dev = bufs[0].engine.device
    g = torch.Generator(device=dev); g.manual_seed(7)
    acts = torch.where(torch.rand((T, N, A), generator=g, device=dev) < 0.7, torch.full((T, N, A), 14, device=dev),
                       torch.randint(0, cfg.n_actions, (T, N, A), generator=g, device=dev)).to(torch.int32)
    learner = dict(rnn_states=torch.randn((T + 1, N, A, 2, 16), generator=g, device=dev), rnn_states_critic=torch.randn((T + 1, N, A, 1, 8), generator=g, device=dev),
                   actions=torch.randint(0, 25, (T, N, A, 1), generator=g, device=dev).float(), action_log_probs=torch.randn((T, N, A, 1), generator=g, device=dev))
    vals = torch.randn((T + 1, N, A, 1), generator=g, device=dev)
    adv = torch.randn((T, N, A, 1), generator=g, device=dev)
    perm_ff = torch.randperm(T * N * A, generator=g, device=dev)
    perm_rec = torch.randperm(T * N * A // L, generator=g, device=dev)
    results = []
    for b in bufs:
        b.collect(acts)                                                   # no synchronize: the generators are enqueued right behind the rollout launch
        b.value_preds.copy_(vals); b.returns.copy_(vals * 2)
        results.append((list(b.feed_forward_generator(adv, 5, learner=learner, perm=perm_ff)),
                        list(b.recurrent_generator(adv, 3, L, learner=learner, perm=perm_rec))))
    torch.cuda.synchronize()
    ref = bufs[0]
    assert int(ref.dones.sum()) > 0                                       # episodes ended inside the rollout (auto-resets)
    arrays = dict(obs=ref.obs, node_obs=ref.node_obs, adj=ref.adj, agent_id=ref.agent_id, masks=ref.masks, active_masks=ref.active_masks,
                  value_preds=ref.value_preds, returns=ref.returns, available_actions=ref.available_actions, advantages=adv, **learner)
    _, _, s_ff = feed_forward_sizes(T, N, A, 5)
    _, _, s_rec = recurrent_sizes(T, N, A, 3, L)
    want_ff = _reference_batches(torch, arrays, True, perm_ff, s_ff)
    want_rec = _reference_batches(torch, arrays, True, perm_rec, s_rec, L)
    for form, (ff, rec) in zip(("rows+materialised", "rows+compact", "table+none"), results):
        for got, want in ((ff, want_ff), (rec, want_rec)):
            assert len(got) == len(want)
            for b, (tup, w) in enumerate(zip(got, want)):
                for k, v in zip(NAMES, tup):
                    assert v.dtype == w[k].dtype and torch.equal(v, w[k]), (form, b, k)
    for b in bufs:
        b.engine.check_errors()


def test_table_form_with_64_or_more_entities():
    import torch
    from gmpe.engine import GmpeEngine
    from gmpe.rollout import DeviceRolloutBuffer
    N, A, T = 3, 32, 5
    cfg = gmpe.make_config(scenario_name=JULY, num_envs=N, num_agents=A, world_size=30.0, episode_length=4, seed=23)
    assert cfg.num_entities >= 64
    bufs = [DeviceRolloutBuffer(GmpeEngine(cfg), T, use_centralized_V=False),
            DeviceRolloutBuffer(GmpeEngine(cfg, adj_compact=True, node_form="table", adj_form="none"), T, use_centralized_V=False)]
    g = torch.Generator(device="cuda"); g.manual_seed(2)
    acts = torch.randint(0, cfg.n_actions, (T, N, A), generator=g, device="cuda", dtype=torch.int32)
    adv = torch.randn((T, N, A, 1), generator=g, device="cuda")
    pf, pr = torch.randperm(T * N * A, generator=g, device="cuda"), torch.randperm(T * N * A // 7, generator=g, device="cuda")
    outs = []
    for b in bufs:
        b.warmup(); b.collect(acts)
        outs.append((list(b.feed_forward_generator(adv, 4, perm=pf)), list(b.recurrent_generator(adv, 2, 7, perm=pr))))
    for x, y in zip(outs[0], outs[1]):
        for tx, ty in zip(x, y):
            for k, u, v in zip(NAMES, tx, ty):
                assert (u is None and v is None) or torch.equal(u, v), k
    ref = bufs[0]
    w = _reference_batches(torch, dict(obs=ref.obs, node_obs=ref.node_obs, adj=ref.adj, agent_id=ref.agent_id, masks=ref.masks,
                                       active_masks=ref.active_masks, advantages=adv, rnn_states=torch.zeros((T + 1, N, A, 1, 1), device="cuda"),
                                       rnn_states_critic=torch.zeros((T + 1, N, A, 1, 1), device="cuda"), actions=adv, action_log_probs=adv,
                                       value_preds=ref.masks, returns=ref.masks, available_actions=ref.masks),
                           False, pf, [(0, T * N * A // 4)])[0]
    for k in ("node_obs", "adj", "obs"):
        assert torch.equal(outs[1][0][0][NAMES.index(k)], w[k]), k
