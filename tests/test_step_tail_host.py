"""CPU side of gmpe_step_tail (include/gmpe.h; gmpe.engine.step_tail): the NumPy restatement the GPU tests compare with (tests/step_tail_lib.py)
against the reference's rules on hand-written dones, the plan's refusals by name before any device call, the wrapper's refusal of host tensors, and
the draw_inc keyword of the policy entries."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import abi_lib
import gmpe
from gmpe import _lib, policy
import step_tail_lib as SL

F32 = np.float32


def _reference_masks(dones_env):
    """graph_mpe_runner.py:395-405 as the runner writes it: dones [N, A] bool"""
    N, A = dones_env.shape
    dones_all = np.all(dones_env, axis=1)
    masks = np.ones((N, A, 1), F32)
    masks[dones_env == True] = np.zeros(((dones_env == True).sum(), 1), F32)      # noqa: E712
    active = np.ones((N, A, 1), F32)
    active[dones_env == True] = np.zeros(((dones_env == True).sum(), 1), F32)     # noqa: E712
    active[dones_all == True] = np.ones(((dones_all == True).sum(), A, 1), F32)   # noqa: E712
    return masks.reshape(-1), active.reshape(-1)


def test_masks_on_hand_written_dones():
    # env 0 partially done, env 1 fully done, env 2 not done; bytes 1 and 255 both count
    d = np.array([[1, 0, 255], [1, 255, 1], [0, 0, 0]], np.uint8)
    m, a = SL.np_masks(d.reshape(-1), 3)
    assert m.tolist() == [0, 1, 0, 0, 0, 0, 1, 1, 1]
    assert a.tolist() == [0, 1, 0, 1, 1, 1, 1, 1, 1]
    rm, ra = _reference_masks(d != 0)
    assert np.array_equal(m, rm) and np.array_equal(a, ra) and m.dtype == a.dtype == F32
    # A = 1: a done agent is its whole env, so it stays active
    m, a = SL.np_masks(np.array([0, 7, 0, 1], np.uint8), 1)
    assert m.tolist() == [1, 0, 1, 0] and a.tolist() == [1, 1, 1, 1]
    rng = np.random.default_rng(0)
    for A in (1, 2, 5):
        d = rng.random((9, A)) < 0.5
        m, a = SL.np_masks(d.reshape(-1), A)
        rm, ra = _reference_masks(d)
        assert np.array_equal(m, rm) and np.array_equal(a, ra)


def test_stop_rows_on_hand_written_dones():
    assert np.array_equal(SL.np_stop_rows(None, 3, 5), np.ones((3, 5), F32))                  # step 0: everything available
    r = SL.np_stop_rows(np.array([0, 255, 1], np.uint8), 3, 5)
    assert r.tolist() == [[1, 1, 1, 1, 1], [0, 0, 1, 0, 0], [0, 0, 1, 0, 0]]                  # available_actions[int(5 / 2)] = 1
    assert SL.np_stop_rows(np.array([1], np.uint8), 1, 4).tolist() == [[0, 0, 1, 0]]
    assert SL.np_stop_rows(np.array([1], np.uint8), 1, 1).tolist() == [[1]]


def test_restatement_writes_the_right_slots_and_nothing_else():
    T, N, A, n, R, H = 3, 2, 2, 5, 1, 2
    lanes = N * A
    dones = np.array([[1, 0, 0, 0, 9], [1, 1, 0, 1, 9], [0, 0, 0, 0, 9]], np.uint8)           # stride 5: one byte of padding
    full = lambda S, w: np.full((S, w + 3), SL.SENTINEL, F32)
    bufs = dict(masks=full(T + 1, lanes), active_masks=full(T + 1, lanes), available_actions=full(T + 1, lanes * n), value_preds=full(T + 1, lanes),
                actions=full(T, lanes), action_log_probs=full(T, lanes), rnn_states=full(T + 1, lanes * R * H))
    ctr = np.array([10], np.uint64)
    ins = dict(_lanes=lanes, values=np.arange(4, dtype=F32), actions=np.array([3, 1, 4, 1], np.int64), action_log_probs=-np.arange(4, dtype=F32),
               rnn_states=np.arange(1, 9, dtype=F32).reshape(4, R, H))
    SL.np_step_tail(1, dones, A, bufs, ins, n=n, counter=ctr, draw_inc=5)
    assert ctr[0] == 15
    assert bufs["masks"][2].tolist() == [0, 0, 1, 0] + [SL.SENTINEL] * 3 and bufs["active_masks"][2, :4].tolist() == [1, 1, 1, 0]
    assert bufs["available_actions"][2, :20].reshape(4, 5).tolist() == [[0, 0, 1, 0, 0]] + [[1] * 5] * 3     # from dones[0], not dones[1]
    assert bufs["value_preds"][1, :4].tolist() == [0, 1, 2, 3] and bufs["actions"][1, :4].tolist() == [3, 1, 4, 1]
    assert bufs["rnn_states"][2, :8].tolist() == [0, 0, 0, 0, 5, 6, 0, 0]
    for name, b in bufs.items():
        touched = {"value_preds": 1, "actions": 1, "action_log_probs": 1}.get(name, 2)
        assert all((b[s] == SL.SENTINEL).all() for s in range(b.shape[0]) if s != touched), name
        assert (b[:, -3:] == SL.SENTINEL).all(), name


def test_symbol_layout_and_abi_version():
    assert "gmpe_step_tail" in _lib.SYMBOLS and "gmpe_step_tail" in abi_lib.exported()
    assert abi_lib.layout(_lib.GmpeStepTailPlan) == abi_lib.mirror_layout(_lib.GmpeStepTailPlan)
    assert abi_lib.constant("GMPE_ABI_VERSION") == 3


def _plan(**kw):
    """A plan that passes every check (never launched here: each test breaks one thing). Pointers are fake, aligned addresses."""
    tp = _lib.GmpeStepTailPlan()
    p = tp.learner
    p.lanes, p.t, p.num_steps, p.recurrent_n, p.hidden, p.hidden_critic, p.act_dim, p.actions_int64 = 40, 2, 5, 1, 64, 64, 1, 1
    for i, name in enumerate(("dones", "values", "actions_in", "log_probs_in", "rnn_in", "rnn_critic_in", "value_preds", "actions", "action_log_probs",
                              "rnn_states", "rnn_states_critic")):
        setattr(p, name, 0x10000000 * (i + 1))
    p.stride_dones, p.stride_value_preds, p.stride_actions, p.stride_action_log_probs = 40, 40, 40, 40
    p.stride_rnn_states = p.stride_rnn_states_critic = 40 * 64
    tp.num_agents, tp.n_actions = 4, 5
    tp.masks, tp.active_masks, tp.available_actions, tp.draw_dev = 0x70000000, 0x71000000, 0x72000000, 0x73000008
    tp.stride_masks, tp.stride_active_masks, tp.stride_available_actions, tp.draw_inc = 40, 40, 200, 1
    for k, v in kw.items():
        setattr(p if hasattr(p, k) else tp, k, v)
    return tp


@pytest.mark.parametrize("bad, msg", [
    # the checks shared with gmpe_insert_learner, under this entry's name
    (dict(lanes=0), b"lanes >= 1"),
    (dict(t=5), b"0 <= t < num_steps"),
    (dict(recurrent_n=65), b"recurrent_n"),
    (dict(act_dim=0), b"act_dim"),
    (dict(reserved=1), b"reserved"),
    (dict(rnn_states=None), b"without its output"),
    (dict(rnn_in=0x10000002), b"misaligned pointer"),
    (dict(stride_rnn_states=40 * 64 - 1), b"overlapping strides"),
    # its own
    (dict(dones=None), b"dones"),
    (dict(dones=None, rnn_in=None, rnn_critic_in=None), b"dones is required"),
    (dict(stride_dones=39, rnn_in=None, rnn_critic_in=None), b"overlapping strides"),
    (dict(num_agents=0), b"num_agents"),
    (dict(num_agents=3), b"lanes % num_agents"),
    (dict(num_agents=-4), b"num_agents"),
    (dict(n_actions=0), b"n_actions"),
    (dict(n_actions=65, stride_available_actions=40 * 65), b"n_actions"),
    (dict(masks=0x70000002), b"misaligned pointer"),
    (dict(available_actions=0x72000001), b"misaligned pointer"),
    (dict(draw_dev=0x73000004), b"misaligned pointer: draw_dev"),
    (dict(stride_masks=39), b"overlapping strides"),
    (dict(stride_masks=0), b"overlapping strides"),
    (dict(stride_active_masks=-40), b"overlapping strides"),
    (dict(stride_available_actions=199), b"overlapping strides"),
])
def test_c_side_refuses_bad_plans_before_any_device_call(bad, msg):
    lib = _lib.load()
    assert lib.gmpe_step_tail(0, C.byref(_plan(**bad)), None) == -1                         # GMPE_ERR_INVALID_ARG
    err = lib.gmpe_last_error()
    assert err.startswith(b"gmpe_step_tail: ") and msg in err, err


def test_c_side_null_plan():
    lib = _lib.load()
    assert lib.gmpe_step_tail(0, None, None) == -1 and lib.gmpe_last_error().startswith(b"gmpe_step_tail: null plan")


def _host_call(**over):
    N, A, T = 3, 2, 5
    z = lambda *s: torch.zeros(s)
    a = dict(step=1, dones=torch.zeros(T, N, A, dtype=torch.uint8),
             arrays=dict(value_preds=z(T + 1, N, A, 1), rnn_states=z(T + 1, N, A, 1, 4)), num_agents=A, masks=z(T + 1, N, A, 1),
             active_masks=z(T + 1, N, A, 1), available_actions=z(T + 1, N, A, 5), values=z(N * A, 1), rnn_states=z(N * A, 1, 4))
    a.update(over)
    step, dones, arrays = a.pop("step"), a.pop("dones"), a.pop("arrays")
    return gmpe.engine.step_tail(step, dones, arrays, **a)


@pytest.mark.parametrize("bad, match", [
    ({}, "no CPU fallback"),                                                              # well-formed host tensors: refused for the device
    (dict(values=None, rnn_states=None), "no CPU fallback"),                              # no learner input: still a launch, still refused
    (dict(step=5), "step"),
    (dict(num_agents=4), "num_agents"),
    (dict(num_agents=0), "num_agents"),
    (dict(masks=torch.zeros(5, 3, 2, 1)), "masks must be a float32 tensor"),
    (dict(active_masks=torch.zeros(6, 3, 2, 1, dtype=torch.float64)), "active_masks must be a float32 tensor"),
    (dict(available_actions=torch.zeros(6, 3, 2, 65)), "n_actions"),
    (dict(available_actions=torch.zeros(6, 3, 2, 10)[..., ::2]), "slot must be contiguous"),
    (dict(rnn_states=torch.zeros(6, 4, 1)), "rnn_states must be a contiguous"),           # insert_learner's checks are the same code
    (dict(draw_dev=torch.zeros(1, dtype=torch.int32)), "draw_dev"),
    (dict(draw_dev=torch.zeros(1, dtype=torch.int64), draw_inc=-1), "draw_inc"),
])
def test_step_tail_refuses_bad_arguments_before_the_device(bad, match):
    with pytest.raises(ValueError, match=match):
        _host_call(**bad)


def test_draw_inc_defaults_to_one_on_the_policy_entries():
    for fn in (policy.actor_forward, policy.get_actions, gmpe.act_head, gmpe.sample_actions):
        p = inspect.signature(fn).parameters["draw_inc"]
        assert p.default == 1 and p.kind is inspect.Parameter.KEYWORD_ONLY, fn
    assert callable(gmpe.engine.step_tail)
