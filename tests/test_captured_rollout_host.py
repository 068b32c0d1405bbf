"""Host side of gmpe.policy.CapturedRollout and run(..., captured=True), no GPU: every refusal and argument check that is specified to happen before the
device is touched, raised on CPU stand-ins as tests/test_value_host.py raises rollout's — what _rollout_buffer refuses, the normaliser compute would
miss, a buffer in mid-episode, an engine whose timing is enabled, a handle on the split big-E path with a dense adjacency —, the captured=True
combinations run refuses as CapturedUpdate refuses them, and the keyword collect_step hands through to the sampling launch."""
import inspect
import types

import pytest
import torch

from gmpe import policy
from gmpe.rollout import DeviceRolloutBuffer
from test_value_host import _fake_buffer


def _engine(**over):
    e = types.SimpleNamespace(N=2, A=3, _timing=False, adj_form="compact", tuning=lambda: {"split": 0}, device=torch.device("cpu"), _ovr=None, _tape=None)
    for k, v in over.items():
        setattr(e, k, v)
    return e


def test_the_names_exist_and_the_defaults_are_todays():
    assert inspect.isclass(policy.CapturedRollout) and callable(policy.CapturedRollout.replay)
    sig = inspect.signature(policy.CapturedRollout.__init__)
    assert list(sig.parameters)[1:6] == ["actor", "critic", "buffer", "value_normalizer", "deterministic"]
    assert sig.parameters["value_normalizer"].default is None and sig.parameters["deterministic"].default is False
    step = inspect.signature(policy.collect_step).parameters["draw_dev"]
    assert step.kind is inspect.Parameter.KEYWORD_ONLY and step.default is None
    assert inspect.signature(policy.run).parameters["captured"].default is False
    assert DeviceRolloutBuffer._act_draw_dev is None and callable(DeviceRolloutBuffer.act_draw_counter)
    assert not hasattr(policy.CapturedRollout, "num_nodes") and "keep_graph" not in sig.parameters


def test_the_buffer_enumerates_its_own_tensors():
    """every tensor attribute, whatever its name, sorted: what CapturedRollout saves, restores and guards; an array added later is in it unlisted"""
    z = torch.zeros(2)
    b = types.SimpleNamespace(obs=z, _adj=z + 1, later_addition=z + 2, engine=object(), step=0, returns=None, _prepared={})
    got = DeviceRolloutBuffer._arrays(b)
    assert [k for k, _ in got] == ["_adj", "later_addition", "obs"] and got[2][1] is z
    b._arrays = types.MethodType(DeviceRolloutBuffer._arrays, b)
    assert [k for k, _ in policy._buffer_arrays(b)] == ["buffer._adj", "buffer.later_addition", "buffer.obs"]


def test_captured_rollout_refuses_before_any_device_call():
    rnn_net, bare_net = types.SimpleNamespace(rnn=object()), types.SimpleNamespace()
    call = lambda b, a=rnn_net, c=rnn_net, vn="vn": policy.CapturedRollout(a, c, b, vn)
    fn = "CapturedRollout"
    # a non-buffer, and what _rollout_buffer refuses of a buffer
    for thing in (object(), None, types.SimpleNamespace(step=0)):
        with pytest.raises(ValueError, match="buffer must be a DeviceRolloutBuffer: %s reads buffer" % fn):
            call(thing)
    with pytest.raises(ValueError, match="%s needs a buffer with value_preds and returns" % fn):
        call(_fake_buffer(value_preds=None))
    with pytest.raises(ValueError, match="%s needs a buffer with value_preds and returns" % fn):
        call(_fake_buffer(returns=None))
    with pytest.raises(ValueError, match="%s reads node_obs rows" % fn):
        call(_fake_buffer(_node_obs=None))
    with pytest.raises(ValueError, match="%s reads an adjacency" % fn):
        call(_fake_buffer(_adj=None))
    with pytest.raises(ValueError, match="the actor has an RNN: %s needs a buffer with rnn_states " % fn):
        call(_fake_buffer(rnn_states=None))
    with pytest.raises(ValueError, match="the critic has an RNN: %s needs a buffer with rnn_states_critic" % fn):
        call(_fake_buffer(rnn_states_critic=None))
    with pytest.raises(ValueError, match="the critic has an RNN"):
        call(_fake_buffer(rnn_states=None, rnn_states_critic=None), a=bare_net)
    # compute's own
    with pytest.raises(ValueError, match="%s needs the runner's args" % fn):
        call(_fake_buffer(args=None))
    with pytest.raises(ValueError, match="%s: args.use_valuenorm / use_popart is set, so a value_normalizer is required" % fn):
        call(_fake_buffer(), vn=None)
    # a buffer in mid-episode
    with pytest.raises(ValueError, match="%s starts at buffer.step == 0, not 2" % fn):
        call(_fake_buffer(step=2, engine=_engine()))
    # the engine: timing, the split big-E path with a dense adjacency
    with pytest.raises(NotImplementedError, match="%s: the engine's timing is enabled.*not supported under capture" % fn):
        call(_fake_buffer(engine=_engine(_timing=True)))
    with pytest.raises(NotImplementedError, match="%s: this handle runs the split big-E path with a dense adjacency.*not supported under capture" % fn):
        call(_fake_buffer(engine=_engine(adj_form="full", tuning=lambda: {"split": 1})))
    # ... which a compact or an absent adjacency does not take, and a handle off that path neither: these get as far as the device check
    for eng in (_engine(tuning=lambda: {"split": 1}), _engine(adj_form="none", tuning=lambda: {"split": 1}), _engine(adj_form="full")):
        with pytest.raises(ValueError, match="no CPU fallback"):
            call(_fake_buffer(engine=eng))


def test_run_refuses_the_captured_combinations_before_anything_else():
    run = lambda **k: policy.run(None, None, None, None, None, None, captured=True, **k)
    with pytest.raises(NotImplementedError, match="install = 'replace': run with captured=True takes \"in_place\" only.*not supported under capture"):
        run(install="replace")
    with pytest.raises(NotImplementedError, match="shards: run with captured=True.*not supported under capture"):
        run(shards=object())
    with pytest.raises(NotImplementedError, match="shards: run with captured=True"):
        run(install="in_place", shards=types.SimpleNamespace(exchange=lambda x: x, world=2, rank=0))
    with pytest.raises(NotImplementedError, match="graph = 'table': run with captured=True takes \"rows\" only.*not supported under capture"):
        run(graph="table")
    # install defaults to "in_place" there: the next refusal is run's own, reached with and without the keyword
    fair = types.SimpleNamespace(increase_fairness=True)
    for kw in ({}, {"install": "in_place"}, {"graph": "rows", "shards": None}):
        with pytest.raises(NotImplementedError, match="args.increase_fairness"):
            policy.run(None, None, None, None, None, fair, captured=True, **kw)
    # ... and what iteration refuses is still refused, by run's name, before the buffer is warmed up
    buf = types.SimpleNamespace(T=6, engine=types.SimpleNamespace(N=4), warmup=lambda: pytest.fail("warmed up"))
    with pytest.raises(NotImplementedError, match="accumulation_steps = 2: run"):
        policy.run(None, None, None, None, buf, types.SimpleNamespace(), captured=True, episodes=1, accumulation_steps=2)
    with pytest.raises(ValueError, match="value_head = 'hip': run"):
        policy.run(None, None, None, None, buf, types.SimpleNamespace(), captured=True, episodes=1, value_head="hip")
    # captured=False is today's run: install="replace" passes through to iteration
    seen = []
    buf.warmup = lambda: None
    import unittest.mock as mock
    with mock.patch.object(policy, "iteration", lambda *a, **k: seen.append(k) or {}):
        policy.run(None, None, None, None, buf, types.SimpleNamespace(), episodes=1, install="replace")
    assert seen == [{"install": "replace"}]


def test_collect_step_hands_the_counter_to_the_sampling_launch(monkeypatch):
    """with draw_dev the draw is the counter's, so the host's act_draw is not baked into the launch: draw = 0; without it, today's call"""
    seen = []

    def get_actions(*a, **k):
        seen.append((k["draw"], k["draw_dev"]))
        return None, None, None, "h", "hc"

    monkeypatch.setattr(policy, "get_actions", get_actions)
    eng = types.SimpleNamespace(N=2, A=3, cfg=types.SimpleNamespace(num_entities=5, seed=1, env_id_base=0))
    b = _fake_buffer(engine=eng, act_draw=7, act_outputs=lambda: {}, act_finish=lambda learner: "out", available_actions_for=lambda t: None,
                     _learner_inputs=lambda *a: None, share_obs=None, obs=None, agent_id=None, share_agent_id=None, masks=None)
    net = types.SimpleNamespace(rnn=object())
    assert policy.collect_step(net, net, b) == "out"
    counter = torch.zeros(1, dtype=torch.int64)
    assert policy.collect_step(net, net, b, draw_dev=counter) == "out"
    assert seen[0] == (7, None) and seen[1][0] == 0 and seen[1][1] is counter
