"""The fixtures of tests/golden/make_trainer_fixture.py — the reference's own GR_MAPPO.ppo_update / train on its own GR_Actor / GR_Critic, float64 —
and tests/trainer_lib.py's mirrors, no GPU:
(a) the mirrors, run through plain torch on the CPU in float64 with torch's own clip_grad_norm_ and Adam in the reference's order, reproduce the
    truth: the same arithmetic in another order. This pins the mirrors, gnn_lib's place in them and trainer_lib's reading of graph_mappo.py to the
    reference's trainer, so that tests/test_gpu_trainer.py holds gmpe.policy to the reference and not to a second reading of it;
(b) the fixture's own conditions, from the stored numbers: err_ref under the cap, no scalar under 1e-2, no file above the largest there was;
(c) the reference's fc_h parameters, and only they, are the ones its Adam never gives state."""
import os

import numpy as np
import pytest
import torch

import trainer_lib as TL

# The largest err of (a) over every array and scalar of every case, measured: 1.21e-15 (the no-clip case's exp_avg_sq). Ten times that:
MIRROR = 1.21e-14


@pytest.mark.parametrize("case", list(TL.CASES))
def test_the_plain_torch_trainer_on_the_mirrors_reproduces_the_references_ppo_update(case):
    fx = TL.load(case)
    scalars, imps, got, _ = TL.run_updates(fx, lambda a, c, ao, co, s, args, vn, ua: TL.torch_ppo_update(a, c, ao, co, s, args, vn, ua), "cpu",
                                           torch.float64)
    TL.compare(fx, scalars, got, TL.SCALARS, case, lambda e_ref: MIRROR, imps)


@pytest.mark.parametrize("case", list(TL.TRAIN_CASES))
def test_the_plain_torch_trainer_on_the_mirrors_reproduces_the_references_train(case):
    fx = TL.load(case)
    info, got = TL.run_train(fx, TL.torch_train, "cpu", torch.float64)
    TL.compare(fx, info, got, TL.TRAIN_INFO, case, lambda e_ref: MIRROR)


def test_the_mirrors_forward_reproduces_the_references():
    fx = TL.inputs()
    actor, critic, _, _, _ = TL.nets(fx, dtype=torch.float64)
    s = TL.sample_on(fx["samples"][0], "cpu", torch.float64)
    with torch.no_grad():
        f, h = actor.features(s[1], s[2], s[3], s[4], s[6], s[11])
        logits = actor.act.action_out.linear(f).masked_fill(s[15] == 0, torch.finfo(torch.float64).min)
        fc, hc = critic.features(s[0], s[2], s[3], s[5], s[7], s[11])
        values = critic.v_out(fc)
    t = fx["forward"]
    actions = logits.argmax(1, keepdim=True)
    assert np.array_equal(actions.numpy(), t["actions"])
    lp = torch.log_softmax(logits, 1).gather(1, actions)
    for k, v in (("action_log_probs", lp), ("rnn_states", h), ("values", values), ("rnn_states_critic", hc)):
        e = TL.err(v.numpy(), t[k])
        print("forward %-18s err %.3g err_ref %.3g" % (k, e, float(t["err_ref:" + k])))
        assert e <= MIRROR and float(t["err_ref:" + k]) <= TL.CAP, k


@pytest.mark.parametrize("case", list(TL.CASES) + list(TL.TRAIN_CASES))
def test_the_fixtures_meet_their_own_conditions(case):
    fx = TL.load(case)
    d, args = fx["raw"], fx["args"]
    t, e = d["scalars"], d["scalars:err_ref"]
    assert float(e.max()) <= TL.CAP and t.shape == ((TL.UPDATES, 6) if case in TL.CASES else (6,))
    names = TL.SCALARS if case in TL.CASES else TL.TRAIN_INFO
    for i in np.ndindex(*t.shape):
        frozen = case == "no-actor" and names[i[-1]] == "actor_grad_norm"
        assert (t[i] == 0.0) if frozen else (abs(t[i]) >= 1e-2), (names[i[-1]], t[i])
    for net in fx["meta"]:
        assert all(fx["err_ref"][net][k] <= TL.CAP for k in TL.KINDS), (net, fx["err_ref"][net])
        m = fx["meta"][net]
        assert len(m["names"]) == len(set(m["names"])) and int(np.sum(m["sizes"])) == fx["truth"][net]["param"].size
        assert fx["truth"][net]["grad"].size == int(np.sum(m["sizes"][m["has_grad"]]))
        assert fx["truth"][net]["exp_avg"].size == fx["truth"][net]["exp_avg_sq"].size == int(np.sum(m["sizes"][m["steps"] > 0]))
    if case in TL.CASES:
        assert float(d["imp_weights:err_ref"]) <= TL.CAP and d["imp_weights"].shape == (TL.UPDATES, TL.ROWS, 1)
        assert sorted(fx["meta"]) == sorted(TL.CASES[case][2])
        col = TL.SCALARS.index
        if args["use_max_grad_norm"]:                   # the clip bites at every update
            assert (t[:, col("critic_grad_norm")] > args["max_grad_norm"]).all()
            assert case == "no-actor" or (t[:, col("actor_grad_norm")] > args["max_grad_norm"]).all()
    else:
        assert len(fx["raw"]["advantages"].shape) == 4 and sum(c[3] for c in TL.ReplayBuffer(fx, "cpu", torch.float32).calls) == 4


def test_no_fixture_file_is_larger_than_the_largest_there_was():
    sizes = {f: os.path.getsize(os.path.join(TL.GOLDEN, f)) for f in TL.files()}
    assert len(sizes) == 28 and max(sizes.values()) <= TL.MAX_FILE, sizes
    assert TL.MAX_FILE == os.path.getsize(os.path.join(TL.GOLDEN, "gru_layer_ones.npz"))


@pytest.mark.parametrize("case", ["plain", "popart", "no-actor", "train-feed-forward"])
def test_fc_h_and_nothing_else_of_a_stepped_network_has_no_state(case):
    fx = TL.load(case)
    for net, m in fx["meta"].items():
        stateless = set(n for n, s in zip(m["names"], m["steps"]) if s == 0)
        graded = set(n for n, g in zip(m["names"], m["has_grad"]) if g)
        fc_h = set(n for n in m["names"] if ".base.mlp.fc_h." in n)
        assert len(fc_h) == 4 and not (fc_h & graded)
        steps = fx["raw"]["scalars"].shape[0] if case in TL.CASES else 4
        assert set(int(s) for s in m["steps"]) == ({0, 1, steps} if case == "popart" else {0, steps})
        if case == "popart":
            # Every PopArt update replaces weight, bias and stddev. The optimiser holds the objects of the first call: stepped once, with the first
            # update's gradients, which the second update's zero_grad() drops; from then on the layer in use is one that nobody trains. The objects
            # the critic holds at the end and the three statistics have neither gradient nor state.
            new = set("critic.v_out." + k for k in ("weight", "bias", "stddev", "mean", "mean_sq", "debiasing_term"))
            old = {"old:critic.v_out.weight", "old:critic.v_out.bias"}
            assert stateless == fc_h | new | {"old:critic.v_out.stddev"} and not ((new | old) & graded)
            assert set(n for n, s in zip(m["names"], m["steps"]) if s == 1) == old
        else:
            assert stateless == fc_h and graded == set(m["names"]) - fc_h
    # the mirror's fc_h is the reference's: loaded strictly, the same four names, and the only parameters the mirror's trainer leaves without state
    actor, critic, aopt, copt, born = TL.nets(fx, case == "popart", recurrent=fx["args"]["use_recurrent_policy"])
    assert sorted(k for k, _ in actor.named_parameters() if ".fc_h." in k) == ["base.mlp.fc_h.0.bias", "base.mlp.fc_h.0.weight", "base.mlp.fc_h.2.bias",
                                                                               "base.mlp.fc_h.2.weight"]
