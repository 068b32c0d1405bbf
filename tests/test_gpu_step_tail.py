"""gmpe_step_tail on the GPU (include/gmpe.h; gmpe.engine.step_tail): the C entry against the NumPy restatement (tests/step_tail_lib.py), bit for bit and
over whole arrays — every array starts as a sentinel, so the padding between slots and the slots beside the written ones are part of every comparison —,
the act entries with draw_inc = 0, and the buffer paths (act_step, insert_step with learner keywords, insert_external, policy.collect_step,
CapturedRollout) against the same steps issued through the still-public pieces in the order the buffer used before: available_actions_for, the
sampling call, engine.step, masks_from_dones, insert_learner.
Mutants of k_step_tail these tests were run against, each an in-bounds change of one rule: the all-done test taken from the workgroup's own lanes only
(6 tests fail: the 33- and 65-lane cases), the stop rows read from dones[t] (22 fail), the masks written into slot t (28 fail)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import gmpe
import gnn_lib as G
import step_tail_lib as SL
from gmpe import _lib, policy
from gmpe.engine import insert_learner, step_tail
from test_gpu_policy import _Net

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _eq(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), what


class _Case(object):
    """The arrays of one gmpe_step_tail problem on the device, each [slots, stride] and filled with the sentinel, with their NumPy twins.
    pad: elements between a slot's rows and the next slot; base_off: floats by which the RNN arrays and inputs start past a 16-byte boundary;
    omit: names of outputs (or learner inputs) left NULL."""

    def __init__(self, N, A, T, n=5, R=1, H=64, Hc=None, k=1, a64=True, byte=1, pad=0, base_off=0, omit=(), seed=0, dones=None):
        self.N, self.A, self.T, self.n, self.R, self.H, self.Hc, self.k, self.a64 = N, A, T, n, R, H, H if Hc is None else Hc, k, a64
        self.lanes, self.pad, self.base_off, self.omit = N * A, pad, base_off, set(omit)
        self.rng = np.random.default_rng(seed)
        L = self.lanes
        if dones is None:
            dones = (self.rng.random((T, L)) < 0.4).astype(np.uint8)
        d = np.full((T, L + pad), 9, np.uint8)                                 # the padding is "done": a read past a slot would show
        d[:, :L] = dones * byte
        self.dones_np, self.dones = d, torch.from_numpy(d).to(DEV)              # slot 0 at the start of its allocation: nothing before dones[0]
        slots = dict(masks=(T + 1, L), active_masks=(T + 1, L), available_actions=(T + 1, L * n), value_preds=(T + 1, L), actions=(T, L * k),
                     action_log_probs=(T, L * k), rnn_states=(T + 1, L * R * H), rnn_states_critic=(T + 1, L * R * self.Hc))
        self.slot = {name: w for name, (_, w) in slots.items()}
        self.flat, self.dev, self.np = {}, {}, {}
        for name, (S, w) in slots.items():
            off = base_off if name.startswith("rnn") else 0
            flat = torch.full((off + S * (w + pad) + 4,), float(SL.SENTINEL), device=DEV)
            self.flat[name] = flat
            self.dev[name] = flat[off:off + S * (w + pad)].view(S, w + pad)
            self.np[name] = np.full((S, w + pad), SL.SENTINEL, np.float32)
        self.counter = torch.tensor([1 << 40], dtype=torch.int64, device=DEV)
        self.counter_np = np.array([1 << 40], np.uint64)

    def inputs(self):
        L, r = self.lanes, self.rng
        f = lambda *s: r.standard_normal(s).astype(np.float32)
        acts = r.integers(0, self.n, (L, self.k))
        return dict(values=f(L, 1), actions=acts.astype(np.int64) if self.a64 else acts.astype(np.float32) + np.float32(0.5),
                    action_log_probs=f(L, self.k), rnn_states=f(L, self.R, self.H), rnn_states_critic=f(L, self.R, self.Hc))

    def to_dev(self, ins):
        out = {}
        for name, x in ins.items():
            off = self.base_off if name.startswith("rnn") else 0
            buf = torch.empty(x.size + 8, dtype=torch.from_numpy(x).dtype, device=DEV)
            v = buf[off:off + x.size].view(x.shape)
            v.copy_(torch.from_numpy(x))
            out[name] = v
        return out

    def plan(self, t, ins_dev, draw_inc=None):
        tp = _lib.GmpeStepTailPlan()
        p, o = tp.learner, self.omit
        p.lanes, p.t, p.num_steps = self.lanes, t, self.T
        p.recurrent_n, p.hidden, p.hidden_critic, p.act_dim, p.actions_int64 = self.R, self.H, self.Hc, self.k, int(self.a64)
        p.dones, p.stride_dones = self.dones.data_ptr(), self.dones.stride(0)
        for name, field, dst in (("values", "values", "value_preds"), ("actions", "actions_in", "actions"),
                                 ("action_log_probs", "log_probs_in", "action_log_probs"), ("rnn_states", "rnn_in", "rnn_states"),
                                 ("rnn_states_critic", "rnn_critic_in", "rnn_states_critic")):
            if name in ins_dev and name not in o:
                setattr(p, field, ins_dev[name].data_ptr())
                setattr(p, dst, self.dev[dst].data_ptr())
                setattr(p, "stride_" + dst, self.dev[dst].stride(0))
        tp.num_agents, tp.n_actions = self.A, self.n
        for name in ("masks", "active_masks"):
            if name not in o:
                setattr(tp, name, self.dev[name].data_ptr())
                setattr(tp, "stride_" + name, self.dev[name].stride(0))
        if "available_actions" not in o:
            tp.available_actions, tp.stride_available_actions = self.dev["available_actions"][1].data_ptr(), self.dev["available_actions"].stride(0)
        if draw_inc is not None:
            tp.draw_dev, tp.draw_inc = self.counter.data_ptr(), draw_inc
        return tp

    def step(self, t, learner=True, draw_inc=None, stream=None):
        """one launch at step t and the same on the twins"""
        ins = self.inputs() if learner else {}
        ins_dev = self.to_dev(ins)
        st = torch.cuda.current_stream() if stream is None else stream
        _lib.check(_lib.load().gmpe_step_tail(0, C.byref(self.plan(t, ins_dev, draw_inc)), C.c_void_p(st.cuda_stream)), "gmpe_step_tail")
        st.synchronize()
        bufs = {k: (None if k in self.omit else v) for k, v in self.np.items()}
        SL.np_step_tail(t, self.dones_np, self.A, bufs, dict({k: v for k, v in ins.items() if k not in self.omit}, _lanes=self.lanes), n=self.n,
                        counter=None if draw_inc is None else self.counter_np, draw_inc=draw_inc or 0)

    def check(self, what):
        torch.cuda.synchronize()
        for name in self.np:
            _eq(self.dev[name].cpu().numpy(), self.np[name], "%s %s" % (what, name))
            edge = self.flat[name].cpu().numpy()
            off = self.base_off if name.startswith("rnn") else 0
            assert (edge[:off] == SL.SENTINEL).all() and (edge[-4:] == SL.SENTINEL).all(), "%s %s: outside the array" % (what, name)
        assert int(self.counter.item()) == int(self.counter_np[0]), what
        _eq(self.dones.cpu().numpy(), self.dones_np, what + " dones")

    def run_all(self, what, **kw):
        for t in range(self.T):
            self.step(t, **kw)
            self.check("%s t=%d" % (what, t))


def _straddle_dones(T=4, N=13, A=5):
    """65 lanes: env 6 has lanes 30 .. 34 around the workgroup boundary at 32, env 12 lanes 60 .. 64 around the one at 64. Done in the first workgroup's
    part only, in the second's only, in both, and the env before it wholly done."""
    d = np.zeros((T, N * A), np.uint8)
    d[0, [30, 31]] = 1; d[0, [60, 61, 62, 63]] = 1
    d[1, [32, 33, 34]] = 1; d[1, 64] = 1
    d[2, 30:35] = 1; d[2, 60:65] = 1
    d[3, 25:30] = 1; d[3, 31] = 1; d[3, 33] = 1
    return d


CASES = {
    "1x1": dict(N=1, A=1, T=1),                                                          # T = 1: t = 0 is also t = T - 1
    "2x3-byte255-n25": dict(N=2, A=3, T=3, n=25, byte=255),
    "11x3-pad": dict(N=11, A=3, T=3, pad=5),                                             # 33 lanes: env 10 straddles, one-lane tail workgroup; strides > slot
    "13x5-straddle": dict(N=13, A=5, T=4, dones=_straddle_dones(), Hc=32),
    "13x5-random-n4-f32-actions": dict(N=13, A=5, T=2, n=4, a64=False, k=2, seed=3),
    "rnn-rows-of-6": dict(N=11, A=3, T=2, R=2, H=3, Hc=5, pad=1),                        # 4-byte path; hidden != hidden_critic
    "rnn-64-off-by-one-float": dict(N=11, A=3, T=2, H=64, base_off=1),                   # a 64-wide row that cannot take the 16-byte path
    "1x1-A1-many": dict(N=70, A=1, T=2, byte=255, n=5),
}


@pytest.mark.parametrize("name", list(CASES))
def test_entry_is_the_restatement_bit_for_bit(name):
    c = _Case(**CASES[name])
    if name == "13x5-straddle":
        a = [SL.np_masks(c.dones_np[t, :65], 5)[1] for t in range(3)]
        assert a[0][30:35].tolist() == [0, 0, 1, 1, 1] and a[1][30:35].tolist() == [1, 1, 0, 0, 0] and a[2][30:35].tolist() == [1] * 5
    c.run_all(name)


@pytest.mark.parametrize("omit", ["masks", "active_masks", "available_actions", "values", "actions", "action_log_probs", "rnn_states",
                                  "rnn_states_critic"])
def test_each_optional_part_alone_left_out(omit):
    c = _Case(N=11, A=3, T=2, omit=(omit,), seed=5)
    c.run_all("without " + omit)
    dst = "value_preds" if omit == "values" else omit
    assert (c.np[dst] == SL.SENTINEL).all()


def test_no_learner_input_still_writes_masks_and_stop_rows():
    c = _Case(N=11, A=3, T=3, seed=6)
    c.run_all("no learner input", learner=False)
    assert (c.np["masks"][1:, :33] != SL.SENTINEL).all() and (c.np["available_actions"][1:, :165] != SL.SENTINEL).all()
    assert (c.np["value_preds"] == SL.SENTINEL).all() and (c.np["rnn_states"] == SL.SENTINEL).all()


def test_counter_on_a_side_stream_and_repeated():
    c = _Case(N=2, A=3, T=2, seed=7)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    for inc in (0, 1, 5, 5, 1, 0):
        c.step(1, draw_inc=inc, stream=side)
    c.check("counter")
    assert int(c.counter.item()) == (1 << 40) + 12


def _tensors(N, A, T, n, R, H, g):
    """the buffer-shaped arrays engine.step_tail takes, and a generator of inputs"""
    z = lambda *s: torch.full(s, float(SL.SENTINEL), device=DEV)
    arrays = dict(value_preds=z(T + 1, N, A, 1), actions=z(T, N, A, 1), action_log_probs=z(T, N, A, 1), rnn_states=z(T + 1, N, A, R, H),
                  rnn_states_critic=z(T + 1, N, A, R, H))
    outs = dict(masks=z(T + 1, N, A, 1), active_masks=z(T + 1, N, A, 1), available_actions=z(T + 1, N, A, n))
    L = N * A
    ins = dict(values=torch.randn((L, 1), generator=g, device=DEV), actions=torch.randint(0, n, (L, 1), generator=g, device=DEV),
               action_log_probs=torch.randn((L, 1), generator=g, device=DEV), rnn_states=torch.randn((L, R, H), generator=g, device=DEV),
               rnn_states_critic=torch.randn((L, R, H), generator=g, device=DEV))
    return arrays, outs, ins


def test_captured_and_replayed_on_changed_dones_and_inputs():
    N, A, T, n, R, H, t = 11, 3, 3, 5, 1, 64, 1
    g = torch.Generator(device=DEV)
    g.manual_seed(1)
    arrays, outs, ins = _tensors(N, A, T, n, R, H, g)
    dones = torch.zeros((T, N, A), dtype=torch.uint8, device=DEV)
    ctr = torch.tensor([3], dtype=torch.int64, device=DEV)
    call = lambda: step_tail(t, dones, arrays, num_agents=A, draw_dev=ctr, draw_inc=1, **outs, **ins)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for rep in range(2):
        dones.copy_((torch.rand((T, N, A), generator=g, device=DEV) < 0.5).to(torch.uint8) * (255 if rep else 1))
        for v in ins.values():
            v.copy_(torch.randint(0, n, v.shape, generator=g, device=DEV) if v.dtype == torch.int64 else torch.randn(v.shape, generator=g, device=DEV))
        for v in list(arrays.values()) + list(outs.values()):
            v.fill_(float(SL.SENTINEL))
        graph.replay()
        torch.cuda.synchronize()
        L = N * A
        bufs = {k: np.full((v.shape[0], v[0].numel()), SL.SENTINEL, np.float32) for k, v in list(arrays.items()) + list(outs.items())}
        SL.np_step_tail(t, dones.cpu().numpy().reshape(T, L), A, bufs, dict({k: v.cpu().numpy() for k, v in ins.items()}, _lanes=L), n=n)
        for k, v in list(arrays.items()) + list(outs.items()):
            _eq(v.cpu().numpy().reshape(v.shape[0], -1), bufs[k], "replay %d %s" % (rep, k))
    assert int(ctr.item()) == 3 + 1 + 2                                          # the warm-up and two replays; the capture itself ran nothing


def test_act_entries_with_draw_inc_zero_leave_the_counter_and_the_outputs():
    import head_lib as HL
    rows, K, A = 70, 25, 5
    g = torch.Generator(device=DEV)
    g.manual_seed(2)
    logits = torch.randn((rows, K), generator=g, device=DEV)
    prev = (torch.rand(rows, generator=g, device=DEV) < 0.3).to(torch.uint8)
    kw = dict(dones_prev=prev, stop_action=K // 2, seed=5, env_id_base=1, num_agents=A, draw=0)
    for call in (lambda **k: gmpe.sample_actions(logits, **kw, **k),
                 lambda f=torch.randn((rows, 64), generator=g, device=DEV), act=HL.act_layer(K, "actor", DEV), **k: gmpe.act_head(f, act, **kw, **k)):
        ctr = torch.tensor([77], dtype=torch.int64, device=DEV)
        one = call(draw_dev=ctr)
        assert int(ctr.item()) == 78
        ctr.fill_(77)
        zero = call(draw_dev=ctr, draw_inc=0)
        assert int(ctr.item()) == 77
        for x, y in zip(one, zero):
            assert (x is None) == (y is None)
            if x is not None:
                _eq(x.cpu().numpy(), y.cpu().numpy(), "draw_inc 0 against 1")


# ---------------------------------------------------------------------------------------------- the buffer paths
N, A, T = 4, 3, 4


def _old_tail(b, t, learner):
    """what followed the env step before: the masks, then the learner fields"""
    b.engine.masks_from_dones(b.dones[t], b.masks[t + 1], b.active_masks[t + 1])
    if learner is not None:
        insert_learner(t, b.dones, b._learner_arrays(), **learner)


def _old_insert_step(b, action_idx, **kw):
    t = b.step
    learner = b._learner_inputs(kw.get("values"), kw.get("actions"), kw.get("action_log_probs"), kw.get("rnn_states"), kw.get("rnn_states_critic"),
                                "insert_step")
    b.available_actions_for(t)
    b._bind(t + 1)
    b.engine.step(action_idx)
    _old_tail(b, t, learner)
    b.step = (t + 1) % b.T


def _old_act_step(b, logits, values, **kw):
    from gmpe.act import sample_actions
    t, e = b.step, b.engine
    c = e.cfg
    learner = b._learner_inputs(values, None, None, kw.get("rnn_states"), kw.get("rnn_states_critic"), "act_step")
    out = b.act_outputs()
    b.available_actions_for(t)
    sample_actions(logits, dones_prev=b.dones[t - 1] if t else None, stop_action=c.n_actions // 2 if t else None, seed=c.seed,
                   env_id_base=c.env_id_base, num_agents=e.A, draw=b.act_draw, out=out)
    b._bind(t + 1)
    e.step(b._act_idx)
    _old_tail(b, t, learner)
    b.act_draw += 1
    b.step = (t + 1) % b.T


def _old_collect_step(actor, critic, b, draw_dev=None):
    t, e = b.step, b.engine
    c, rows = e.cfg, e.N * e.A
    s = policy._slot_rows(b, t)
    out = b.act_outputs()
    out["values"] = b.value_preds[t]
    b.available_actions_for(t)
    _, _, _, h, hc = policy.get_actions(actor, critic, s["share_obs"], s["obs"], s["node_obs"], s["adj"], s["agent_id"], s["share_agent_id"],
                                        s["rnn_states"], s["rnn_states_critic"], s["masks"], None, False,
                                        dones_prev=b.dones[t - 1].view(rows) if t else None, seed=c.seed, env_id_base=c.env_id_base, num_agents=e.A,
                                        draw=b.act_draw if draw_dev is None else 0, draw_dev=draw_dev, out=out)
    learner = b._learner_inputs(None, None, None, h if hasattr(actor, "rnn") else None, hc if hasattr(critic, "rnn") else None, "collect_step")
    b._bind(t + 1)
    e.step(b._act_idx)
    _old_tail(b, t, learner)
    b.act_draw += 1
    b.step = (t + 1) % b.T


def _twins(avail, rnn, args=None):
    from gmpe.engine import GmpeEngine
    from gmpe.rollout import DeviceRolloutBuffer
    cfg = gmpe.make_config(num_envs=N, num_agents=A, episode_length=3, seed=11)       # the time limit lies inside the rollout: dones occur
    engines = [GmpeEngine(cfg, device=0) for _ in range(2)]
    pf = ("value_preds", "returns", "advantages") + (("available_actions",) if avail else ())
    lf = ("actions", "action_log_probs") + (("rnn_states", "rnn_states_critic") if rnn else ())
    bufs = [DeviceRolloutBuffer(e, T, use_centralized_V=False, policy_fields=pf, learner_fields=lf, args=args, recurrent_N=1, hidden_size=64)
            for e in engines]
    for b in bufs:
        b.warmup()
    return cfg, engines, bufs


def _same_buffers(ba, bb, what):
    torch.cuda.synchronize()
    na, nb = dict(ba._arrays()), dict(bb._arrays())
    assert sorted(na) == sorted(nb) and "masks" in na and "dones" in na, what
    na.pop("_ws", None)                                    # compute_returns' scratch: torch.empty, and no step writes it
    for k in na:
        _eq(na[k].cpu().numpy(), nb[k].cpu().numpy(), "%s %s" % (what, k))
    assert ba.act_draw == bb.act_draw and ba.step == bb.step, what
    sa, sb = ba.engine.get_state(), bb.engine.get_state()
    assert type(sa) is type(sb)
    for k in (sa if isinstance(sa, dict) else range(len(sa))):
        x, y = sa[k], sb[k]
        if isinstance(x, torch.Tensor):
            _eq(x.cpu().numpy(), y.cpu().numpy(), "%s engine state %s" % (what, k))
        elif isinstance(x, np.ndarray):
            _eq(x, y, "%s engine state %s" % (what, k))


@pytest.mark.parametrize("avail", [True, False], ids=["avail", "no-avail"])
@pytest.mark.parametrize("rnn", [True, False], ids=["rnn", "no-rnn"])
def test_act_step_and_insert_step_are_the_pieces_in_the_old_order(avail, rnn):
    cfg, engines, (ba, bb) = _twins(avail, rnn)
    g = torch.Generator(device=DEV)
    g.manual_seed(4)
    L, K = N * A, int(cfg.n_actions)
    for ep in range(2):
        for t in range(T):
            vals = torch.randn((L, 1), generator=g, device=DEV)
            states = dict(rnn_states=torch.randn((L, 1, 64), generator=g, device=DEV),
                          rnn_states_critic=torch.randn((L, 1, 64), generator=g, device=DEV)) if rnn else {}
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                if t % 2 == 0:
                    logits = torch.randn((L, K), generator=g, device=DEV)
                    ba.act_step(logits, vals, **states)
                    _old_act_step(bb, logits, vals, **states)
                else:
                    action = torch.randint(0, K, (L, 1), generator=g, device=DEV)
                    kw = dict(values=vals, actions=action, action_log_probs=torch.randn((L, 1), generator=g, device=DEV), **states)
                    ba.insert_step(action.view(N, A).to(torch.int32), **kw)
                    _old_insert_step(bb, action.view(N, A).to(torch.int32), **kw)
            finally:
                torch.cuda.set_sync_debug_mode("default")
            _same_buffers(ba, bb, "episode %d step %d" % (ep, t))
        assert bool(ba.dones.any())
        for b in (ba, bb):
            b.after_update()
        _same_buffers(ba, bb, "after_update %d" % ep)
    for e in engines:
        e.check_errors()
        e.close()


@pytest.mark.parametrize("avail", [True, False], ids=["avail", "no-avail"])
def test_insert_external_is_the_pieces_in_the_old_order(avail):
    cfg, engines, (ba, bb) = _twins(avail, True)
    g = torch.Generator(device=DEV)
    g.manual_seed(8)
    L = N * A
    z = lambda x: torch.zeros_like(x[0])
    for ep in range(2):
        for t in range(T):
            dones = (torch.rand((N, A), generator=g, device=DEV) < 0.5).to(torch.uint8)
            kw = dict(values=torch.randn((L, 1), generator=g, device=DEV), actions=torch.randint(0, 5, (L, 1), generator=g, device=DEV),
                      action_log_probs=torch.randn((L, 1), generator=g, device=DEV), rnn_states=torch.randn((L, 1, 64), generator=g, device=DEV),
                      rnn_states_critic=torch.randn((L, 1, 64), generator=g, device=DEV))
            ba.insert_external(z(ba.obs), z(ba.agent_id), z(ba._node_obs), z(ba._adj), z(ba.rewards), dones, **kw)
            assert bb.step == t
            learner = bb._learner_inputs(kw["values"], kw["actions"], kw["action_log_probs"], kw["rnn_states"], kw["rnn_states_critic"], "insert_external")
            bb.available_actions_for(t)
            for dst, src in ((bb.obs[t + 1], z(bb.obs)), (bb.agent_id[t + 1], z(bb.agent_id)), (bb._node_obs[t + 1], z(bb._node_obs)),
                             (bb._adj[t + 1], z(bb._adj)), (bb.rewards[t], z(bb.rewards)), (bb.dones[t], dones)):
                dst.copy_(src)
            _old_tail(bb, t, learner)
            bb.step = (t + 1) % T
            _same_buffers(ba, bb, "episode %d step %d" % (ep, t))
        for b in (ba, bb):
            b.after_update()
    for e in engines:
        e.close()


def _nets(cfg, engines, rnn):
    F = int(cfg.node_feats)
    key = G.ACTOR if F == 7 else G.ROTATE
    actor = _Net(key, engines[0].D, "act").to(DEV)
    critic = _Net(key, 0, "v_out", use_cent_obs=False, seed=12).to(DEV)
    if not rnn:
        del actor.rnn, critic.rnn
    return actor, critic


ARGS = types.SimpleNamespace(gamma=0.99, gae_lambda=0.95, use_gae=True, use_proper_time_limits=False, use_valuenorm=False, use_popart=False)


@pytest.mark.parametrize("avail", [True, False], ids=["avail", "no-avail"])
@pytest.mark.parametrize("rnn", [True, False], ids=["rnn", "no-rnn"])
def test_collect_step_is_the_pieces_in_the_old_order(avail, rnn):
    cfg, engines, (ba, bb) = _twins(avail, rnn, ARGS)
    actor, critic = _nets(cfg, engines, rnn)
    ca, cb = ba.act_draw_counter(), bb.act_draw_counter()
    policy.collect_step(actor, critic, ba)                                         # every kernel's one-time attribute call, outside the sync check
    _old_collect_step(actor, critic, bb)
    for b in (ba, bb):
        b.warmup()
        b.act_draw = 0
        b.sync_act_draw_counter()
    for ep in range(2):
        for t in range(T):
            counted = t % 2 == 1                                                   # every other step keys its draw by the device counter
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                policy.collect_step(actor, critic, ba, draw_dev=ca if counted else None)
                _old_collect_step(actor, critic, bb, draw_dev=cb if counted else None)
                if not counted:
                    ca += 1                                                        # the host's act_draw moved: keep the counters equal to it
                    cb += 1
            finally:
                torch.cuda.set_sync_debug_mode("default")
            _same_buffers(ba, bb, "episode %d step %d" % (ep, t))
            assert int(ca.item()) == ba.act_draw == int(cb.item()), (ep, t)
        assert bool(ba.dones.any())
        for b in (ba, bb):
            b.after_update()
    for e in engines:
        e.check_errors()
        e.close()


def test_captured_rollout_replayed_twice_is_the_eager_rollout():
    cfg, engines, (ba, bb) = _twins(True, True, ARGS)
    actor, critic = _nets(cfg, engines, True)
    cap = policy.CapturedRollout(actor, critic, ba)
    for ep in range(2):
        cap.replay()
        policy.rollout(actor, critic, bb)
        _same_buffers_but_counter(ba, bb, "episode %d" % ep)
        assert int(ba.act_draw_counter().item()) == ba.act_draw == bb.act_draw == (ep + 1) * T
        for b in (ba, bb):
            b.after_update()
    for e in engines:
        e.check_errors()
        e.close()


def _same_buffers_but_counter(ba, bb, what):
    """bb never asked for a device counter: give it one holding what the captured side's must hold"""
    bb.act_draw_counter()
    bb.sync_act_draw_counter()
    _same_buffers(ba, bb, what)
