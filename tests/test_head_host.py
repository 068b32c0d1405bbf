"""Host side of the policy's action head (include/gmpe.h gmpe_head_forward / gmpe_head_backward / gmpe_act_head, gmpe.action_logits / gmpe.act_head,
gmpe.policy), no GPU:
(a) the float32 run of tests/head_lib.py's formulas stays under the 1e-5 cap for every array of every accuracy case; the fixture's keys and shapes and
    the parameter reader;
(b) the exported symbols, the plan's layout against the C header, the workspace size against the restated geometry, the refusals of both layers;
(c) the compiler's resource report of csrc/gmpe_head.hip shows no scratch memory."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import abi_lib
import gmpe
import head_lib as HL
from gmpe import _lib

MB = 1 << 20


# ---------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("case", HL.CASES, ids=HL.case_id)
def test_the_float32_run_of_the_formulas_stays_under_the_cap(case):
    f, w, b, g, t64, e_ref = HL.truth(case)
    for k in HL.ARRAYS:
        print("%s %-14s err_ref %.3g" % (HL.case_id(case), k, e_ref[k]))
    for k in HL.ARRAYS:
        assert e_ref[k] <= HL.CAP, (case, k, e_ref[k])
    assert np.abs(t64["logits"]).max() > 0 and np.abs(t64["grad_weight"]).max() > 0


def test_the_cases_are_the_listed_ones():
    have = set(HL.CASES)
    assert len(have) == len(HL.CASES)
    for K in (1, 5, 24, 25, 64):
        for rows in (1, 65, 255, 256, 257, 513, 4097):
            assert (rows, K, "random") in have
    assert (257, 25, "actor") in have and (4097, 25, "rotate") in have
    assert {K | 1 == K for K in HL.KS} == {True, False}                             # S = K and S = K + 1
    assert HL.partition(4097) == (128, 33) and HL.partition(1) == (1, 1) and HL.partition(33) == (2, 17)


def test_the_fixture_holds_the_shipped_names_and_shapes():
    g = HL.golden()
    for tag in ("actor", "rotate"):
        assert g[tag + ".act.action_out.linear.weight"].shape == (25, 64) and g[tag + ".act.action_out.linear.bias"].shape == (25,)
    assert g["critic.v_out.weight"].shape == (1, 64) and g["critic.v_out.bias"].shape == (1,) and g["critic.v_out.stddev"].shape == (1,)
    assert all(v.dtype == np.float32 for v in g.values()) and len(g) == 7
    assert not np.array_equal(g["actor.act.action_out.linear.weight"], g["rotate.act.action_out.linear.weight"])


def test_the_parameter_reader_reads_the_three_forms():
    from gmpe import head as W
    for source in ("actor", "rotate"):
        act = HL.act_layer(25, source)
        lin = act.action_out.linear
        for obj, path in ((act, "act.action_out.linear"), (act.action_out, "act.linear"), (lin, "act")):
            p, w, b = W._head_params(obj, "action_logits")
            assert p == path and w is lin.weight and b is lin.bias
        assert np.array_equal(lin.weight.detach().numpy(), HL.golden()[source + ".act.action_out.linear.weight"])
        assert tuple(lin.weight.shape) == (25, 64) and tuple(lin.bias.shape) == (25,)


# ---------------------------------------------------------------------------------------------- (b)
def test_symbols_are_exported_and_the_plan_matches_the_header():
    lib = _lib.load()
    assert {"gmpe_head_workspace_bytes", "gmpe_head_forward", "gmpe_head_backward", "gmpe_act_head"} <= set(_lib.SYMBOLS) & abi_lib.exported()
    assert lib.gmpe_abi_version() == 3 and gmpe.config.ABI_VERSION == 3          # added entry points: the ABI version stays
    assert abi_lib.layout(_lib.GmpeHeadPlan) == abi_lib.mirror_layout(_lib.GmpeHeadPlan) and C.sizeof(_lib.GmpeHeadPlan) == 8 + 2 * 4 + 10 * 8
    assert [abi_lib.constant("GMPE_PPO_MAX_ACTIONS"), abi_lib.constant("GMPE_ABI_VERSION")] == [64, 3] and gmpe.head.MAX_ACTIONS == 64 and gmpe.head.HIDDEN == 64
    assert ("int", "gmpe_act_head", ["int", "const gmpe_act_plan*", "const gmpe_head_plan*", "void*"]) in abi_lib.prototypes()
    assert gmpe.action_logits is gmpe.head.action_logits and gmpe.act_head is gmpe.head.act_head
    assert gmpe.head_workspace_bytes is gmpe.head.head_workspace_bytes
    for name in ("actor_forward", "critic_forward", "minibatch_losses", "evaluator_act"):
        assert callable(getattr(gmpe.policy, name))


def test_workspace_bytes_and_the_restated_geometry():
    lib = _lib.load()
    n = C.c_size_t(7)
    assert lib.gmpe_head_workspace_bytes(100, 25, 0, C.byref(n)) == 0 and n.value == 0                  # the forward-only plan takes none
    want = {1: 1 * 32768 + 512, 32: 1 * 32768 + 512, 33: 2 * 32768 + 512, 4096: 128 * 32768 + 16 * 512, 4097: 128 * 32768 + 17 * 512}
    for rows in (1, 32, 33, 4096, 4097, 255, 256, 257, 40960, 512000):
        for K in (1, 25, 64):                                                       # the size depends on rows alone
            assert lib.gmpe_head_workspace_bytes(rows, K, 1, C.byref(n)) == 0
            assert n.value == HL.workspace_bytes(rows) == gmpe.head_workspace_bytes(rows, K) and n.value % 8 == 0, (rows, K)
            assert gmpe.head_workspace_bytes(rows, K, backward=False) == 0
        if rows in want:
            assert n.value == want[rows], rows
    for args, field in (((0, 25, 1), "rows"), ((-3, 25, 1), "rows"), (((1 << 40) + 1, 25, 1), "rows"), ((10, 0, 1), "n_actions"), ((10, 65, 1), "n_actions"),
                        ((10, 25, 2), "want_backward")):
        assert lib.gmpe_head_workspace_bytes(*args, C.byref(n)) == -1
        msg = lib.gmpe_last_error().decode()
        assert msg.startswith("gmpe_head_workspace_bytes:") and field in msg, msg
    assert lib.gmpe_head_workspace_bytes(10, 25, 1, None) == -1 and "bytes_out" in lib.gmpe_last_error().decode()
    with pytest.raises(ValueError, match="n_actions = 65"):
        gmpe.head_workspace_bytes(10, 65)


PTRS = ("features", "weight", "bias", "logits_out", "grad_logits", "grad_features", "grad_weight", "grad_bias", "workspace")


def _plan(**over):
    """a head plan over fake, well separated addresses: nothing here reaches a device"""
    p = _lib.GmpeHeadPlan()
    p.rows, p.n_actions, p.hidden, p.workspace_bytes = 70, 25, 64, 64 * MB
    for i, k in enumerate(PTRS):
        setattr(p, k, (i + 1) * MB)
    for k, v in over.items():
        setattr(p, k, v)
    return p


def _act_plan(**over):
    p = _lib.GmpeActPlan()
    p.rows, p.n_actions, p.num_agents, p.stop_action = 70, 25, 7, 12
    p.action_idx, p.log_probs = 20 * MB, 21 * MB
    for k, v in over.items():
        setattr(p, k, v)
    return p


def _refused(fn, args, *names):
    lib = _lib.load()
    assert getattr(lib, fn)(0, *args, None) == -1
    msg = lib.gmpe_last_error().decode()
    assert msg.startswith(fn + ":") and all(n in msg for n in names), msg


@pytest.mark.parametrize("fn", ["gmpe_head_forward", "gmpe_head_backward"])
def test_c_entry_points_refuse_bad_plans_before_any_device_call(fn):
    bwd = fn == "gmpe_head_backward"
    _refused(fn, (None,), "null plan")
    for bad, name in ((dict(rows=0), "rows"), (dict(rows=(1 << 40) + 1), "rows"), (dict(n_actions=0), "n_actions"), (dict(n_actions=65), "n_actions"),
                      (dict(hidden=32), "hidden"), (dict(hidden=128), "hidden"), (dict(features=MB + 2), "features"), (dict(weight=MB + 1), "weight"),
                      (dict(bias=MB + 3), "bias"), (dict(logits_out=MB + 2), "logits_out"), (dict(grad_logits=MB + 2), "grad_logits"),
                      (dict(grad_features=MB + 1), "grad_features"), (dict(grad_weight=MB + 2), "grad_weight"), (dict(grad_bias=MB + 2), "grad_bias"),
                      (dict(workspace=5 * MB + 4), "workspace")):
        _refused(fn, (C.byref(_plan(**bad)),), name)
    for k in (("features", "weight", "grad_logits", "workspace") if bwd else ("features", "weight", "bias", "logits_out")):
        _refused(fn, (C.byref(_plan(**{k: None})),), k, "required")
    if bwd:
        _refused(fn, (C.byref(_plan(workspace_bytes=HL.workspace_bytes(70) - 8)),), "workspace_bytes", str(HL.workspace_bytes(70)))


def test_the_fused_entry_refuses_what_either_plan_gets_wrong():
    fn = "gmpe_act_head"
    ok = lambda **o: C.byref(_plan(**o))
    _refused(fn, (None, ok()), "null plan")
    _refused(fn, (C.byref(_act_plan()), None), "null head_plan")
    _refused(fn, (C.byref(_act_plan(logits=30 * MB)), ok()), "logits must be NULL")
    for bad, name in ((dict(rows=0), "rows"), (dict(n_actions=65), "n_actions"), (dict(num_agents=0), "num_agents"), (dict(stop_action=25), "stop_action"),
                      (dict(deterministic=2), "deterministic"), (dict(reserved=1), "reserved"), (dict(action_idx=None), "action_idx"),
                      (dict(log_probs=None), "log_probs"), (dict(available_actions=MB, dones_prev=2 * MB), "at most one"),
                      (dict(actions_i64=MB + 4), "8-byte")):
        _refused(fn, (C.byref(_act_plan(**bad)), ok()), name)
    for bad, name in ((dict(hidden=32), "hidden"), (dict(features=None), "features"), (dict(weight=None), "weight"), (dict(bias=None), "bias"),
                      (dict(logits_out=MB + 1), "logits_out"), (dict(rows=71), "head_plan->rows"), (dict(n_actions=24), "head_plan->n_actions")):
        _refused(fn, (C.byref(_act_plan()), ok(**bad)), name)


def test_what_each_entry_point_does_not_need_may_be_null():
    """a forward-only plan: no gradient pointers, no workspace; a backward plan: no bias, no logits_out, any of the three outputs; the fused entry: no
    logits_out. The plans pass the host's checks and fail at the first device call (there is no device here): the error is not an argument error."""
    lib = _lib.load()
    if torch.cuda.is_available():
        return                                          # fake addresses must not reach a real device
    grads = {k: None for k in ("grad_logits", "grad_features", "grad_weight", "grad_bias", "workspace")}
    assert lib.gmpe_head_forward(0, C.byref(_plan(workspace_bytes=0, **grads)), None) == -2, lib.gmpe_last_error().decode()
    assert lib.gmpe_head_backward(0, C.byref(_plan(bias=None, logits_out=None, grad_features=None, grad_bias=None)), None) == -2
    assert lib.gmpe_act_head(0, C.byref(_act_plan()), C.byref(_plan(logits_out=None, workspace_bytes=0, **grads)), None) == -2


def test_python_layer_refuses_what_it_does_not_support():
    z = torch.zeros
    f = z(10, 64)
    act = HL.act_layer(25)
    kw = dict(seed=1, num_agents=2, draw=0)
    for call in (lambda *a, **k: gmpe.action_logits(*a), lambda *a, **k: gmpe.act_head(*a, **k)):
        # NotImplementedError: what is not built
        bad = HL.act_layer(25)
        bad.multi_discrete = True
        with pytest.raises(NotImplementedError, match="multi_discrete"):
            call(f, bad, **kw)
        bad = HL.act_layer(25)
        bad.mixed_action = True
        with pytest.raises(NotImplementedError, match="mixed_action"):
            call(f, bad, **kw)
        bad = types.SimpleNamespace(action_outs=[act.action_out], multi_discrete=False, mixed_action=False)
        with pytest.raises(NotImplementedError, match="action_outs"):
            call(f, bad, **kw)
        gauss = type("DiagGaussian", (torch.nn.Module,), {})()
        gauss.fc_mean = torch.nn.Linear(64, 2)
        with pytest.raises(NotImplementedError, match="DiagGaussian"):
            call(f, types.SimpleNamespace(action_out=gauss), **kw)
        bern = type("Bernoulli", (torch.nn.Module,), {})()
        bern.linear = torch.nn.Linear(64, 2)
        with pytest.raises(NotImplementedError, match="Bernoulli"):
            call(f, types.SimpleNamespace(action_out=bern), **kw)
        for dt in (torch.float16, torch.bfloat16):
            with pytest.raises(NotImplementedError, match="actor_features is .*float32 only"):
                call(f.to(dt), act, **kw)
            with pytest.raises(NotImplementedError, match=r"act.action_out.linear.weight is .*float32 only"):
                call(f, HL.act_layer(25).to(dt), **kw)
        with pytest.raises(NotImplementedError, match="H = 32"):
            call(z(10, 32), torch.nn.Linear(32, 25), **kw)
        with pytest.raises(NotImplementedError, match="hidden = 64"):
            call(z(10, 32), act, **kw)
        # ValueError: what is malformed
        with pytest.raises(ValueError, match=r"act.action_out.linear is missing"):
            call(f, types.SimpleNamespace(action_out=torch.nn.Module()), **kw)
        with pytest.raises(ValueError, match="linear is missing"):
            call(f, types.SimpleNamespace(), **kw)
        with pytest.raises(ValueError, match="K = 65"):
            call(f, torch.nn.Linear(64, 65), **kw)
        with pytest.raises(ValueError, match="actor_features must be contiguous"):
            call(z(64, 10).t(), act, **kw)
        with pytest.raises(ValueError, match="actor_features must be a tensor"):
            call(None, act, **kw)
        with pytest.raises(ValueError, match="actor_features must be float32"):
            call(f.double(), act, **kw)
        with pytest.raises(ValueError, match="actor_features must have shape"):
            call(z(10, 2, 64), act, **kw)
        with pytest.raises(ValueError, match="bias is missing"):
            call(f, torch.nn.Linear(64, 25, bias=False), **kw)
        # everything else in order: the arrays are not on a device (an ACTLayer, a Categorical, an nn.Linear)
        for obj in (act, act.action_out, act.action_out.linear):
            with pytest.raises(ValueError, match="no CPU fallback"):
                call(f, obj, **kw)
    # act_head: sample_actions' own refusals, in its words with the features as the anchor
    with pytest.raises(ValueError, match="at most one"):
        gmpe.act_head(f, act, z(10, 25), dones_prev=z(10, dtype=torch.uint8), **kw)
    with pytest.raises(ValueError, match="stop_action is read with dones_prev only"):
        gmpe.act_head(f, act, stop_action=3, **kw)
    with pytest.raises(ValueError, match="unknown out entries"):
        gmpe.act_head(f, act, out={"values": z(10)}, **kw)
    with pytest.raises(ValueError, match=r"out\['logits'\] must be a contiguous torch.float32 tensor with 250 elements"):
        gmpe.act_head(f, act, out={"logits": z(10, 24)}, **kw)
    with pytest.raises(ValueError, match="num_agents must be >= 1"):
        gmpe.act_head(f, act, seed=1, num_agents=0, draw=0)
    # the composition lets a layer's refusal through: several ids per row (critic_graph_aggr == "node") is gnn_base's
    with pytest.raises(ValueError, match="16-tuple"):
        gmpe.policy.minibatch_losses(None, None, (1, 2, 3), None)


# ---------------------------------------------------------------------------------------------- (c)
def test_no_kernel_of_the_file_uses_scratch_memory():
    assert "head" in abi_lib.ru_objects()                                                           # `make resource-usage` holds it
    names, scratch = list(abi_lib.kernels("head")), list(abi_lib.scratch("head", "k_head").values())
    assert len(names) == len(scratch) == 5 and all(s == 0 for s in scratch), (names, scratch)       # forward, the fused rollout form, backward's three
    for k in ("k_head_fwd", "k_head_act", "k_head_bwd_rows", "k_head_wgrad", "k_head_finish"):
        assert any(k in n for n in names), k
