"""Mixed-batch replay of the reference's own rollouts (tests/golden/*_A*_s*.npz) — test helper, not a conftest.

One batch of N envs holds the fixture's env at several env indices ("fixture slots": env 0, the last lane of the first tile, a
middle lane of an interior tile, env N - 1 in a partial last tile) and random distractor envs everywhere else (their own RNG
tape rows and actions). The batch is driven through one launch path of the GPU engine:
  "step"      one eng.step() per step (FL = 0 / 1 instantiations),
  "rollout"   eng.rollout() into slot-per-step storage with masks and active masks (FL = 2), in segments that end at each
              reset step of the fixture (guided fixtures inject the reference's positions after a reset, on the host),
  "step_many" eng.step_many() over the same segments (FL = 2, final outputs only).
Every step (every segment end where only that is observable) each fixture slot is compared with the reference's recorded
outputs and state, post-reset state included, and every env with the CPU oracle (test_gpu_parity._compare_step /
_compare_state). With eng=None the oracle itself is the subject: the CPU check of the harness (tests/test_oracle_golden.py).
"""
import os

import numpy as np

import gmpe

JULY = "nav_metered_one_goal_graph_rotate_tube_july"
TOL = 1e-5
OUT_KEYS = ("obs", "agent_id", "node_obs", "adj", "reward", "done", "info")


def is_rot(path):
    """rot_inv family fixtures (rot_inv / two_phase / three_phase): cooldown and prev_proj are recorded."""
    return not os.path.basename(path).startswith("july")


def fixture_config(d, path, num_envs, seed=1):
    name = str(d["scenario_name"]) if is_rot(path) else JULY          # the July fixtures predate the name field
    return gmpe.make_config(scenario_name=name, num_envs=num_envs, num_agents=int(d["A"]), world_size=float(d["world_size"]),
                            episode_length=int(d["episode_length"]), max_speed=float(d["max_speed"]),
                            collision_rew=float(d["collision_rew"]), formation_rew=float(d["formation_rew"]), goal_rew=float(d["goal_rew"]),
                            graph_feat_type=str(d["graph_feat_type"]) if "graph_feat_type" in d else "relative",
                            formation_type=str(d["formation_type"]) if "formation_type" in d else "point", seed=seed)


def fixture_slots(N, G):
    """Env 0, the last lane of a tile (the first tile's when that lane is not env 0's neighbour, else the first such tile's), a middle lane of
    an interior tile, env N - 1 (in a partial last tile when G does not divide N). No two of them are neighbours: identical envs never
    sit side by side in a tile."""
    tiles = (N + G - 1) // G
    last = next(k * G - 1 for k in range(1, tiles + 1) if k * G - 1 >= 2)
    mid = (tiles // 2) * G + G // 2
    while mid - last < 2:
        mid += 1
    out = [0, last, mid, N - 1]
    assert all(b - a >= 2 for a, b in zip(out, out[1:])), (N, G, out)
    return out


def spread_slots(N, n):
    """n env indices spread over [0, N), the last one N - 1."""
    return sorted({int(round(q)) for q in np.linspace(0, N - 1, n)} | {N - 1})


class MixedBatch(object):
    def __init__(self, path, num_envs, slots, seed=0, tape_len=4096, steps=None):
        d = self.d = np.load(path)
        self.path, self.N, self.slots = path, num_envs, list(slots)
        assert len(set(self.slots)) == len(self.slots) and max(self.slots) < num_envs
        self.rot = is_rot(path)
        self.T = int(d["T"]) if steps is None else int(steps)
        assert self.T <= int(d["T"])
        self.cfg = fixture_config(d, path, num_envs, seed=seed + 1)
        self.A, self.E = int(d["A"]), int(d["E"])
        rng = np.random.RandomState(1000 + seed)
        ftape = np.asarray(d["tape"], dtype=np.float64)
        self.tape = rng.rand(num_envs, max(tape_len, len(ftape)))        # distractors: their own draws; the fixture row past its end: never read
        self.tape[self.slots, :len(ftape)] = ftape
        self.acts = rng.randint(0, self.cfg.n_actions, (self.T, num_envs, self.A)).astype(np.int32)
        self.acts[:, self.slots] = np.asarray(d["act"][:self.T], dtype=np.int32)[:, None]
        self.guided = bool(d["guided"])
        self.did_reset = np.asarray(d["did_reset"][:self.T], dtype=bool)
        self.n_inj = self.n_reset = 0
        self.checked_resets = 0

    # ------------------------------------------------------------------ setup
    def prepare(self, tgt):
        """Tape and initial prev_phase of every env, then the reset; returns its outputs."""
        pp = tgt.get("prev_phase").copy()
        pp[self.slots] = self.d["init_prev_phase"]
        tgt.set("prev_phase", pp)
        tgt.set_tape(self.tape)
        return tgt.reset()

    def start(self, sub, orc=None):
        """Tape, initial prev_phase, reset, the reset-0 check, the first injection: on the subject and the oracle alike."""
        d = self.d
        outs = [_outputs(self.prepare(tgt)) for tgt in ([sub] if orc is None else [sub, orc])]
        o = outs[0]
        for n in self.slots:
            np.testing.assert_allclose(o["obs"][n], d["reset0_obs"], rtol=0, atol=TOL, err_msg="reset0 obs env %d" % n)
            np.testing.assert_allclose(o["node_obs"][n], d["reset0_node"], rtol=0, atol=TOL, err_msg="reset0 node env %d" % n)
            np.testing.assert_allclose(o["adj"][n], np.broadcast_to(d["reset0_adj"], o["adj"][n].shape), rtol=0, atol=TOL, err_msg="reset0 adj env %d" % n)
            np.testing.assert_array_equal(o["agent_id"][n], d["reset0_id"])
        self._check_placement(sub, "reset0_", None, "reset0")
        if orc is not None:
            _oracle_state(sub, orc, "reset")
        if self.guided:
            self._inject(sub, orc)

    def _inject(self, sub, orc):
        inj = self.d["inject"][self.n_inj]
        self.n_inj += 1
        for tgt in ([sub] if orc is None else [sub, orc]):
            for f, c in (("x", 0), ("y", 1), ("s2", 2), ("s3", 3)):
                v = tgt.get(f).copy()
                v[self.slots] = inj[:, c]
                tgt.set(f, v)

    # ------------------------------------------------------------------ checks against the reference
    def check_outputs(self, o, t, label=""):
        """Fixture slots vs the reference's returned outputs of step t (post-reset ones on a reset step)."""
        d = self.d
        K = d["info"].shape[-1]                       # 17 keys in the July files, 18 (+Phase_reached) in the rot_inv family
        for n in self.slots:
            lab = "%s t=%d env %d" % (label, t, n)
            np.testing.assert_allclose(o["reward"][n], d["rew"][t], rtol=0, atol=TOL, err_msg=lab + " rew")
            np.testing.assert_array_equal(o["done"][n].astype(bool), d["done"][t], err_msg=lab + " done")
            np.testing.assert_allclose(o["obs"][n], d["ret_obs"][t], rtol=0, atol=TOL, err_msg=lab + " obs")
            np.testing.assert_allclose(o["node_obs"][n], d["ret_node"][t], rtol=0, atol=TOL, err_msg=lab + " node")
            ref = np.broadcast_to(d["ret_adj"][t], o["adj"][n].shape)
            np.testing.assert_allclose(o["adj"][n], ref, rtol=0, atol=TOL, err_msg=lab + " adj")
            np.testing.assert_array_equal(o["adj"][n] == 0, ref == 0, err_msg=lab + " adj zero pattern")
            np.testing.assert_allclose(o["info"][n][:, :K], d["info"][t], rtol=2e-6, atol=2e-5, err_msg=lab + " info")

    def check_state(self, sub, t, label=""):
        """Fixture slots vs the reference's state after step t: the stepped state, or on a reset step the post-reset one (before injection)."""
        d = self.d
        ctr = sub.get("rng_ctr")
        for n in self.slots:
            assert ctr[n] == d["tape_pos"][t + 1], "%s draw count t=%d env %d: %d vs %d" % (label, t, n, ctr[n], d["tape_pos"][t + 1])
        if self.did_reset[t]:
            self._check_placement(sub, "rs_", self.n_reset, "%s reset t=%d" % (label, t))
            pp = sub.get("prev_phase")
            for n in self.slots:
                np.testing.assert_array_equal(pp[n], d["rs_prev_phase"][self.n_reset], err_msg="%s rs prev_phase env %d" % (label, n))
            self.n_reset += 1
            self.checked_resets += 1
            return
        st = {f: sub.get(f) for f in ("x", "status", "prev_phase", "phase_reached") + (("cooldown", "prev_proj") if self.rot else ())}
        for n in self.slots:
            lab = "%s t=%d env %d" % (label, t, n)
            np.testing.assert_allclose(st["x"][n], d["st_x"][t], rtol=0, atol=2e-6, err_msg=lab + " x")
            np.testing.assert_array_equal(st["status"][n].astype(bool), d["st_status"][t], err_msg=lab + " status")
            np.testing.assert_array_equal(st["prev_phase"][n], d["st_prev_phase"][t], err_msg=lab + " prev_phase")
            np.testing.assert_array_equal(st["phase_reached"][n], d["st_phase_reached"][t], err_msg=lab + " phase_reached")
            if self.rot:
                np.testing.assert_array_equal(st["cooldown"][n], d["st_cooldown"][t], err_msg=lab + " cooldown")
                np.testing.assert_allclose(st["prev_proj"][n], d["st_prev_proj"][t], rtol=0, atol=2e-6, err_msg=lab + " prev_proj")

    def _check_placement(self, sub, prefix, idx, label):
        check_placement(sub, self.d, prefix, idx, self.slots, label)

    def after_step(self, sub, orc, t):
        """State checks after step t, then the host-side injection of a guided fixture's reset."""
        self.check_state(sub, t)
        if orc is not None:
            _oracle_state(sub, orc, "t=%d" % t)
        if self.did_reset[t] and self.guided:
            self._inject(sub, orc)

    def segments(self):
        """[t0, t1] step ranges that end at each reset step (inclusive) and at the last step."""
        ends = [t for t in range(self.T) if self.did_reset[t]]
        if not ends or ends[-1] != self.T - 1:
            ends.append(self.T - 1)
        out, t0 = [], 0
        for t1 in ends:
            out.append((t0, t1)); t0 = t1 + 1
        return out

    def finish(self, sub):
        assert self.checked_resets == int(self.did_reset.sum())
        assert not sub.get("error_flags").any()


class OracleBatch(object):
    """A batch with no reference env (navigation_graph has no reference rollout): the same launch paths as MixedBatch, every env against
    the oracle only (Philox draws keyed by the config's seed, random actions, segments of `seg` steps)."""

    def __init__(self, cfg, T, seg, seed=0):
        self.cfg, self.N, self.A, self.T, self.seg = cfg, cfg.num_envs, cfg.num_agents, T, seg
        self.acts = np.random.RandomState(2000 + seed).randint(0, cfg.n_actions, (T, self.N, self.A)).astype(np.int32)

    def start(self, sub, orc):
        _oracle_step_reset(sub.reset(), orc.reset(), self.cfg)
        _oracle_state(sub, orc, "reset")

    def check_outputs(self, o, t, label=""):
        pass

    def after_step(self, sub, orc, t):
        _oracle_state(sub, orc, "t=%d" % t)

    def segments(self):
        return [(t0, min(t0 + self.seg, self.T) - 1) for t0 in range(0, self.T, self.seg)]

    def finish(self, sub):
        assert not sub.get("error_flags").any()


def _oracle_step_reset(eo, oo, cfg):
    np.testing.assert_allclose(eo.obs.cpu().numpy(), oo[0], rtol=0, atol=TOL, err_msg="reset obs")
    np.testing.assert_allclose(eo.node_obs.cpu().numpy(), oo[2], rtol=0, atol=TOL, err_msg="reset node")
    adj = eo.adj.cpu().numpy()
    np.testing.assert_allclose(adj, np.broadcast_to(oo[3][:, None], adj.shape), rtol=0, atol=TOL, err_msg="reset adj")


def run_outputs(eng, mb, path_kind):
    """Drive mixed batch mb through one launch path ("step" or "rollout") with no checks; the guided fixture's injections happen after the
    same steps as in replay_on_gpu. Returns every step's outputs ({key: [T, ...] tensor}, masks included on the rollout path) and the
    final state: what the bit-identity comparisons between instantiations read."""
    import torch
    mb.prepare(eng)
    if mb.guided:
        mb.n_inj = 0
        mb._inject(eng, None)
    T = mb.T
    st = {k: torch.zeros((T,) + tuple(getattr(eng.out, k).shape), dtype=getattr(eng.out, k).dtype, device="cuda") for k in OUT_KEYS}
    if path_kind == "step":
        for t in range(T):
            o = eng.step(torch.as_tensor(mb.acts[t], device="cuda"))
            for k in OUT_KEYS:
                st[k][t].copy_(getattr(o, k))
            if mb.did_reset[t] and mb.guided:
                mb._inject(eng, None)
    else:
        assert path_kind == "rollout", path_kind
        from gmpe.engine import StepOutputs
        slot0 = StepOutputs(**{k: st[k][0] for k in OUT_KEYS})
        strides = {k: st[k][0].numel() for k in OUT_KEYS}
        for t0, t1 in mb.segments():
            eng.rollout(torch.as_tensor(mb.acts[t0:t1 + 1], device="cuda"), t1 - t0 + 1, slot0=slot0, num_slots=T, first_slot=t0, strides=strides)
            if mb.did_reset[t1] and mb.guided:
                mb._inject(eng, None)
    torch.cuda.synchronize()
    eng.check_errors()
    return st, eng.get_state()


def check_placement(sub, d, prefix, idx, slots, label):
    """Placement (x / y / theta / speed) and tube record of envs `slots` vs the fixture's reset0_* (idx None) or rs_*[idx], at
    test_oracle_golden's tolerances (_check_tube's layout)."""
    g = lambda k: d[prefix + k] if idx is None else d[prefix + k][idx]
    x, y, th, sp, tube, lm = (sub.get(f) for f in ("x", "y", "s2", "s3", "tube", "landmarks"))
    for n in slots:
        lab = "%s env %d" % (label, n)
        np.testing.assert_allclose(x[n], g("x"), rtol=0, atol=1e-14, err_msg=lab + " x")
        np.testing.assert_allclose(y[n], g("y"), rtol=0, atol=1e-14, err_msg=lab + " y")
        np.testing.assert_allclose(th[n], g("theta"), rtol=0, atol=1e-14, err_msg=lab + " theta")
        np.testing.assert_allclose(sp[n], g("speed"), rtol=0, atol=1e-14, err_msg=lab + " speed")
        tb = tube[n]
        np.testing.assert_allclose(tb[0], g("tube_angle"), rtol=0, atol=1e-15, err_msg=lab + " tube_angle")
        np.testing.assert_allclose(tb[1:3], g("entrance"), rtol=0, atol=1e-14, err_msg=lab + " entrance")
        np.testing.assert_allclose(tb[3:5], g("exit"), rtol=0, atol=1e-14, err_msg=lab + " exit")
        np.testing.assert_allclose(tb[5:7], g("tube_e"), rtol=0, atol=1e-14, err_msg=lab + " tube_e")
        np.testing.assert_array_equal(tb[7:9].astype(np.float32), g("tube_n").astype(np.float32), err_msg=lab + " tube_n")
        np.testing.assert_allclose(tb[9], g("tube_L"), rtol=0, atol=1e-14, err_msg=lab + " tube_L")
        np.testing.assert_allclose(tb[10], g("half_w"), rtol=0, atol=1e-15, err_msg=lab + " half_w")
        np.testing.assert_allclose(tb[11], g("width"), rtol=0, atol=1e-15, err_msg=lab + " width")
        np.testing.assert_allclose(lm[n], g("landmarks"), rtol=0, atol=1e-14, err_msg=lab + " landmarks")


def _outputs(o):
    """Outputs as numpy: an oracle tuple (adj [N,E,E] -> [N,1,E,E]) or the engine's StepOutputs / a dict of slot tensors."""
    if isinstance(o, tuple):
        out = dict(obs=o[0], agent_id=o[1], node_obs=o[2], adj=o[3][:, None])
        if len(o) > 4:                                # a step (a reset returns the first four)
            out.update(reward=o[4], done=o[5], info=o[6])
        return out
    get = o.__getitem__ if isinstance(o, dict) else (lambda k: getattr(o, k))
    return {k: get(k).detach().cpu().numpy() for k in OUT_KEYS}


def _oracle_state(eng, orc, label):
    from test_gpu_parity import _compare_state
    _compare_state(eng, orc, label)


def _oracle_step(eo, oo, cfg, label):
    from test_gpu_parity import _compare_step
    _compare_step(eo, oo, cfg.num_entities, cfg.num_agents, label)


class _View(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def replay_on_oracle(path, num_envs, slots, seed=0):
    """The harness with the CPU oracle as the subject: every fixture slot of the mixed batch must reproduce the reference."""
    import oracle_lib as ol
    mb = MixedBatch(path, num_envs, slots, seed=seed)
    orc = ol.Oracle(mb.cfg)
    mb.start(orc)
    for t in range(mb.T):
        mb.check_outputs(_outputs(orc.step(mb.acts[t])), t, "oracle")
        mb.after_step(orc, None, t)
    mb.finish(orc)
    orc.close()
    return mb


def replay_on_gpu(eng, mb, path_kind):
    """Drive the mixed batch mb through one launch path of the GPU engine eng (created for mb.cfg); fixture slots vs the reference,
    every env vs the oracle. Returns the oracle's number of env resets."""
    import torch
    import oracle_lib as ol
    orc = ol.Oracle(mb.cfg)
    mb.start(eng, orc)
    N, A, T = mb.N, mb.A, mb.T
    n_resets = 0
    if path_kind == "step":
        for t in range(T):
            eo = eng.step(torch.as_tensor(mb.acts[t], device="cuda"))
            oo = orc.step(mb.acts[t])
            n_resets += int(oo[7].sum())
            mb.check_outputs(_outputs(eo), t, "step")
            _oracle_step(eo, oo, mb.cfg, "step t=%d" % t)
            mb.after_step(eng, orc, t)
    else:
        assert path_kind in ("rollout", "step_many"), path_kind
        if path_kind == "rollout":
            st = {k: torch.zeros((T,) + tuple(getattr(eng.out, k).shape), dtype=getattr(eng.out, k).dtype, device="cuda") for k in OUT_KEYS}
            st["masks"] = torch.full((T, N, A), -1.0, device="cuda")
            st["active"] = torch.full((T, N, A), -1.0, device="cuda")
            from gmpe.engine import StepOutputs
            slot0 = StepOutputs(**{k: st[k][0] for k in OUT_KEYS})
            strides = {k: st[k][0].numel() for k in OUT_KEYS}
            strides["masks"] = N * A
        for t0, t1 in mb.segments():
            K = t1 - t0 + 1
            acts = torch.as_tensor(mb.acts[t0:t1 + 1], device="cuda")
            if path_kind == "rollout":
                eng.rollout(acts, K, slot0=slot0, num_slots=T, first_slot=t0, strides=strides, masks=st["masks"], active_masks=st["active"])
            else:
                eo = eng.step_many(acts, K)
            torch.cuda.synchronize()
            for t in range(t0, t1 + 1):
                oo = orc.step(mb.acts[t])
                n_resets += int(oo[7].sum())
                if path_kind == "rollout":
                    view = _View(**{k: st[k][t] for k in OUT_KEYS})
                    mb.check_outputs(_outputs(view.__dict__), t, "rollout")
                    _oracle_step(view, oo, mb.cfg, "rollout t=%d" % t)
                    d = torch.as_tensor(oo[5], device="cuda")
                    alld = d.all(dim=1, keepdim=True)
                    assert torch.equal(st["masks"][t], (~d).float()), ("masks", t)                      # graph_buffer.py:223-251
                    assert torch.equal(st["active"][t], (~(d & ~alld)).float()), ("active_masks", t)
                elif t == t1:
                    mb.check_outputs(_outputs(eo), t, "step_many")
                    _oracle_step(eo, oo, mb.cfg, "step_many t=%d" % t)
            mb.after_step(eng, orc, t1)
    mb.finish(eng)
    eng.check_errors()
    orc.close()
    return n_resets
