"""CPU side of the learner's fields of the device rollout buffer (include/gmpe.h gmpe_insert_learner, DeviceRolloutBuffer learner_fields): the storage spec
and its initial values, the exported symbol and plan layout, the argument checks of the C entry point and of the Python wrappers before any launch, and
the NumPy restatement (tests/learner_lib.py) the GPU tests rely on, against the reference's own vectors (tests/golden/learner_buffer_*.npz)."""
import argparse
import ctypes as C
import glob
import os
import types

import numpy as np
import pytest
import torch

import abi_lib
import gmpe
from gmpe import _lib
from gmpe.rollout import LEARNER_FIELDS, DeviceRolloutBuffer, learner_storage_spec
import learner_lib as LL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FIXTURES = sorted(glob.glob(os.path.join(GOLD, "learner_buffer_*.npz")))


class _HostEngine(object):
    """What DeviceRolloutBuffer.__init__ reads from an engine, on the host (no GPU): enough to see which arrays it allocates."""

    def __init__(self, cfg):
        self.cfg, self.device, self.adj_compact = cfg, torch.device("cpu"), True
        self.node_form, self.adj_form = "rows", "compact"
        self.N, self.A = cfg.num_envs, cfg.num_agents
        self.out = types.SimpleNamespace(info=None)

    def tuning(self):
        return dict(roll=1, split=0)


def _cfg():
    return gmpe.make_config(num_envs=4, num_agents=3, episode_length=5)


def test_learner_storage_spec_shapes():
    cfg = _cfg()
    N, A, T = 4, 3, 6
    f32 = torch.float32
    assert LEARNER_FIELDS == ("rnn_states", "rnn_states_critic", "actions", "action_log_probs")
    assert learner_storage_spec(cfg, T) == {"rnn_states": (f32, (T + 1, N, A, 1, 64)), "rnn_states_critic": (f32, (T + 1, N, A, 1, 64)),
                                            "actions": (f32, (T, N, A, 1)), "action_log_probs": (f32, (T, N, A, 1))}
    spec = learner_storage_spec(cfg, T, ("rnn_states_critic", "actions"), recurrent_N=2, hidden_size=8, hidden_size_critic=16, act_dim=3)
    assert spec == {"rnn_states_critic": (f32, (T + 1, N, A, 2, 16)), "actions": (f32, (T, N, A, 3))}
    with pytest.raises(ValueError, match="unknown learner"):
        learner_storage_spec(cfg, T, ("values",))
    with pytest.raises(ValueError, match=">= 1"):
        learner_storage_spec(cfg, T, recurrent_N=0)


def test_buffer_learner_fields_shapes_sizes_and_zero_initial_values():
    cfg = _cfg()
    N, A, T = 4, 3, 6
    args = argparse.Namespace(recurrent_N=2, hidden_size=8)
    buf = DeviceRolloutBuffer(_HostEngine(cfg), T, learner_fields="all", args=args)
    shapes = dict(rnn_states=(T + 1, N, A, 2, 8), rnn_states_critic=(T + 1, N, A, 2, 8), actions=(T, N, A, 1), action_log_probs=(T, N, A, 1))
    for k in LEARNER_FIELDS:
        t = getattr(buf, k)
        assert tuple(t.shape) == shapes[k] and t.dtype == torch.float32 and t.is_contiguous()
        assert float(t.abs().max()) == 0.0 and not torch.signbit(t).any()                 # graph_buffer.py:114-154: np.zeros
    assert buf.value_preds is None                                                         # policy_fields="all" / learner_fields are separate
    assert len(buf._carried()) == 8                                                        # + rnn_states, rnn_states_critic
    # keyword overrides win over args; with neither, the reference's argparse defaults (recurrent_N 1, hidden_size 64)
    b2 = DeviceRolloutBuffer(_HostEngine(cfg), T, learner_fields=("rnn_states",), args=args, hidden_size=16, recurrent_N=1)
    assert tuple(b2.rnn_states.shape) == (T + 1, N, A, 1, 16) and b2.rnn_states_critic is None and b2.actions is None
    b3 = DeviceRolloutBuffer(_HostEngine(cfg), T, learner_fields=("rnn_states_critic",), hidden_size_critic=5)
    assert tuple(b3.rnn_states_critic.shape) == (T + 1, N, A, 1, 5)
    # a storage entry requests its field; policy_fields="all" keeps today's five fields only
    mine = torch.full((T, N, A, 1), 3.0)
    b4 = DeviceRolloutBuffer(_HostEngine(cfg), T, policy_fields="all", storage={"action_log_probs": mine})
    assert b4.action_log_probs is mine and b4.actions is None and b4.rnn_states is None and b4.value_preds is not None
    assert float(mine.max()) == 3.0                                                        # caller storage is not cleared (zeros are the caller's)
    with pytest.raises(ValueError, match="storage\\['actions'\\]"):
        DeviceRolloutBuffer(_HostEngine(cfg), T, storage={"actions": torch.zeros(T + 1, N, A, 1)})
    with pytest.raises(ValueError, match="unknown learner"):
        DeviceRolloutBuffer(_HostEngine(cfg), T, learner_fields=("values",))


def test_buffer_without_learner_fields_keeps_todays_storage():
    cfg = _cfg()
    T = 6
    for kw in ({}, dict(policy_fields="all", args=argparse.Namespace(recurrent_N=2, hidden_size=8))):
        buf = DeviceRolloutBuffer(_HostEngine(cfg), T, **kw)
        for k in LEARNER_FIELDS:
            assert getattr(buf, k) is None
        assert len(buf._carried()) == (6 if not kw else 8)                                # bad_masks, available_actions with policy_fields
        assert not set(LEARNER_FIELDS) & {k for k, v in buf.minibatch_arrays().items() if v is not None}
    own = {k: v.shape for k, v in vars(DeviceRolloutBuffer(_HostEngine(cfg), T)).items() if isinstance(v, torch.Tensor)}
    assert sorted(own) == ["_adj", "_node_obs", "active_masks", "agent_id", "dones", "masks", "obs", "rewards"]


def test_insert_keywords_refuse_fields_the_buffer_does_not_keep():
    cfg = _cfg()
    N, A, T = 4, 3, 6
    buf = DeviceRolloutBuffer(_HostEngine(cfg), T, learner_fields=("actions",))
    z = lambda *s: torch.zeros(s)
    for kw, match in ((dict(rnn_states=z(N * A, 1, 64)), "rnn_states.*learner_fields"), (dict(action_log_probs=z(N * A, 1)), "action_log_probs"),
                      (dict(values=z(N * A, 1), actions=torch.zeros(N * A, 1, dtype=torch.int64)), "value_preds.*policy_fields")):
        with pytest.raises(ValueError, match=match):
            buf.insert_step(torch.zeros(N, A, dtype=torch.int32), **kw)                     # refused before the env step: the host engine cannot step
        with pytest.raises(ValueError, match=match):
            buf.insert_external(None, None, None, None, None, None, **kw)
    assert buf.step == 0


def test_new_symbol_is_exported_and_bound():
    assert "gmpe_insert_learner" in _lib.SYMBOLS and "gmpe_insert_learner" in abi_lib.exported()      # bound: tests/test_abi_host.py, for every symbol


def test_learner_plan_layout_matches_c_header():
    assert abi_lib.layout(_lib.GmpeLearnerPlan) == abi_lib.mirror_layout(_lib.GmpeLearnerPlan)
    from gmpe.config import ABI_VERSION
    assert abi_lib.constant("GMPE_ABI_VERSION") == 3 == ABI_VERSION                          # additive: the ABI version is unchanged


def _plan(**kw):
    """A plan that passes every check (never launched here: each test breaks one thing). Pointers are fake, aligned addresses."""
    p = _lib.GmpeLearnerPlan()
    p.lanes, p.t, p.num_steps, p.recurrent_n, p.hidden, p.hidden_critic, p.act_dim, p.actions_int64 = 40, 2, 5, 1, 64, 64, 1, 1
    for i, name in enumerate(("dones", "values", "actions_in", "log_probs_in", "rnn_in", "rnn_critic_in", "value_preds", "actions", "action_log_probs",
                              "rnn_states", "rnn_states_critic")):
        setattr(p, name, 0x10000000 * (i + 1))
    p.stride_dones, p.stride_value_preds, p.stride_actions, p.stride_action_log_probs = 40, 40, 40, 40
    p.stride_rnn_states = p.stride_rnn_states_critic = 40 * 64
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("bad, msg", [
    (dict(lanes=0), b"lanes >= 1"),
    (dict(lanes=-3), b"lanes >= 1"),
    (dict(t=5), b"0 <= t < num_steps"),
    (dict(t=-1), b"0 <= t < num_steps"),
    (dict(num_steps=0, t=0), b"num_steps >= 1"),
    (dict(recurrent_n=0), b"recurrent_n"),
    (dict(recurrent_n=65), b"recurrent_n"),
    (dict(hidden=0), b"hidden"),
    (dict(hidden_critic=70000), b"hidden"),
    (dict(act_dim=0), b"act_dim"),
    (dict(act_dim=65), b"act_dim"),
    (dict(actions_int64=2), b"actions_int64"),
    (dict(reserved=1), b"reserved"),
    (dict(rnn_states=None), b"without its output"),
    (dict(value_preds=None), b"without its output"),
    (dict(dones=None), b"need dones"),
    (dict(rnn_in=0x10000002), b"misaligned pointer"),
    (dict(action_log_probs=0x20000001), b"misaligned pointer"),
    (dict(actions_in=0x30000004), b"misaligned pointer"),                                # int64 actions need 8-byte alignment
    (dict(stride_rnn_states=40 * 64 - 1), b"overlapping strides"),
    (dict(stride_rnn_states_critic=0), b"overlapping strides"),
    (dict(stride_actions=39), b"overlapping strides"),
    (dict(stride_value_preds=-40), b"overlapping strides"),
    (dict(stride_dones=39), b"overlapping strides"),
])
def test_c_side_refuses_bad_plans_before_any_device_call(bad, msg):
    lib = _lib.load()
    assert lib.gmpe_insert_learner(0, C.byref(_plan(**bad)), None) == -1                    # GMPE_ERR_INVALID_ARG
    err = lib.gmpe_last_error()
    assert err.startswith(b"gmpe_insert_learner: ") and msg in err, err


def test_c_side_null_plan_and_unused_fields():
    lib = _lib.load()
    assert lib.gmpe_insert_learner(0, None, None) == -1 and b"null plan" in lib.gmpe_last_error()
    # a field that is not given is not checked: values only needs value_preds and its stride; no input at all is a no-op without any device call
    p = _plan(rnn_in=None, rnn_critic_in=None, values=None, actions_in=None, log_probs_in=None, hidden=0, recurrent_n=0, act_dim=0, stride_rnn_states=0)
    assert lib.gmpe_insert_learner(0, C.byref(p), None) == 0


def _dev_arrays(T=5, N=3, A=2, R=1, H=4):
    z = lambda *s: torch.zeros(s)
    return dict(value_preds=z(T + 1, N, A, 1), actions=z(T, N, A, 1), action_log_probs=z(T, N, A, 1), rnn_states=z(T + 1, N, A, R, H),
                rnn_states_critic=z(T + 1, N, A, R, H))


@pytest.mark.parametrize("bad, match", [
    (dict(step=5), "step"),
    (dict(dones=torch.zeros(5, 3, 2, dtype=torch.int32)), "dones"),
    (dict(arrays=dict(rnn_states=torch.zeros(6, 3, 2, 1, 4), returns=torch.zeros(6, 3, 2, 1))), "unknown learner arrays"),
    (dict(arrays=dict(value_preds=torch.zeros(6, 3, 2, 1))), "actions given without the actions array"),
    (dict(arrays=dict(_dev_arrays(), rnn_states=torch.zeros(5, 3, 2, 1, 4))), "rnn_states must hold 6 slots"),
    (dict(arrays=dict(_dev_arrays(), rnn_states=torch.zeros(6, 3, 2, 1, 4, dtype=torch.float64))), "rnn_states must be a float32"),
    (dict(arrays=dict(_dev_arrays(), rnn_states=torch.zeros(6, 3, 2, 1, 8)[..., ::2])), "slot must be contiguous"),
    (dict(rnn_states=torch.zeros(6, 1, 8)[:, :, ::2]), "rnn_states must be a contiguous"),           # a strided input
    (dict(rnn_states=torch.zeros(6, 4, 1)), "rnn_states must be a contiguous"),                       # R, H swapped
    (dict(actions=torch.zeros(6, 1, dtype=torch.int32)), "actions must be a contiguous"),
    (dict(action_log_probs=torch.zeros(6, 2)), "action_log_probs must be a contiguous"),
    (dict(values=torch.zeros(7)), "values must be a contiguous"),
    ({}, "CUDA"),                                                                                    # well-formed host tensors: refused for the device
])
def test_insert_learner_refuses_bad_arguments_before_launch(bad, match):
    N, A = 3, 2
    a = dict(step=1, dones=torch.zeros(5, N, A, dtype=torch.uint8), arrays=_dev_arrays(),
             values=torch.zeros(N * A, 1), actions=torch.zeros(N * A, 1, dtype=torch.int64), action_log_probs=torch.zeros(N * A, 1),
             rnn_states=torch.zeros(N * A, 1, 4), rnn_states_critic=torch.zeros(N * A, 1, 4))
    a.update(bad)
    with pytest.raises(ValueError, match=match):
        gmpe.engine.insert_learner(**a)


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_numpy_restatement_is_the_reference_bit_for_bit(path):
    d = np.load(path)
    T, N, A, R, H = (int(d[k]) for k in ("T", "N", "A", "R", "H"))
    got = LL.np_insert(d, T, N, A, R, H)
    for k, v in got.items():
        assert v.dtype == d["buf_" + k].dtype == np.float32
        np.testing.assert_array_equal(v.view(np.uint32), d["buf_" + k].view(np.uint32), err_msg=k)
    after = LL.np_after_update(got)
    for k, v in after.items():
        np.testing.assert_array_equal(v.view(np.uint32), d["after_" + k].view(np.uint32), err_msg=k)
    dn = d["in_dones"]
    assert dn.all(-1).any() and (dn.any(-1) & ~dn.all(-1)).any()                          # whole-env and single-agent dones both occur
    assert (d["in_rnn_states"][dn] != 0).all()                                             # the zeros come from the rule, not from the inputs


def test_both_fixture_shapes_are_present():
    names = sorted(os.path.basename(p) for p in FIXTURES)
    assert names == ["learner_buffer_R1_H64_central.npz", "learner_buffer_R2_H8_decentral.npz"]
