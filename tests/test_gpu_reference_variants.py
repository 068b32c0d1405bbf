"""The reference's own rollouts (tests/golden/*_A*_s*.npz) through every fused-kernel instantiation of the four tube scenario variants.

env_kernel<SC> (csrc/gmpe_sc.hip) is the one place that picks k_env<BLOCK, AP, SC, FL, GC> from the plan. VARIANTS lists every
(BLOCK, AP, FL, GC) it can return, with the GMPE_* knobs, launch path and fixture shape that reach it; each row is crossed with
July, rot_inv, two_phase and three_phase and replayed as a mixed batch (tests/replay_lib.py): the fixture's env in several env slots
of a batch of random distractors, every fixture slot against the reference every step (segment ends on the rollout paths, reset-step
placement included), every env against the oracle. Every case replays a guided fixture, so phases 1 -> 2, goal arrival and a reset
happen inside the kernel under test. navigation_graph (no reference rollout exists) runs the same rows against the oracle alone, and
test_instantiations_are_bit_identical holds the rows of one scenario to each other bit for bit. tests/test_host_logic.py::
test_every_instantiation_has_a_variant_row fails on the CPU when libgmpe.so grows an instantiation without a row here.

The bench-shape tests run the launches bench.py times for c3 / c3r / c3p2 / c3p3 (4096 x 10; those workloads are exactly the configs
of the fixtures named in BENCH_FIXTURES) with the fixture in eight env slots spread across the batch, env 4095 included.
"""
import os

import pytest

import gmpe
import replay_lib as R

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCEN = ("july", "rotinv", "twophase", "threephase")
# guided fixtures of each scenario by agent count: A = 10 selects the exact-size instantiations (AP = 10), A = 3 AP = 3, A = 6 run-time sizes
FIXTURES = {
    "july": {"A10": "july_A10_s5_guided", "A3": "july_A3_s2_guided", "A6": "july_A6_s4_guided"},
    "rotinv": {"A10": "rotinv_A10_s12_guided", "A3": "rotinv_A3_s9_guided", "A6": "rotinv_A6_s11_guided"},
    "twophase": {"A10": "twophase_A10_s26_guided", "A3": "twophase_A3_s23_guided", "A6": "twophase_A6_s25_guided"},
    "threephase": {"A10": "threephase_A10_s46_guided", "A3": "threephase_A3_s43_guided", "A6": "threephase_A6_s45_guided"},
}

# (BLOCK, AP, FL, GC) -> the ways a tube-scenario batch reaches it: knobs (GMPE_<name>), launch path ("step": FL = 0 / 1, "rollout" /
# "step_many": FL = 2), fixture shape, and the tuning() fields that make env_kernel return that instantiation (asserted before the replay).
# FL = 1 runs for step launches with nt = 0, spec = 1 on BLOCK 256, AP 10 tiles (launch_env); GC = 4 / 6 when the tile holds exactly that many envs.
VARIANTS = {
    (64, 0, 0, 0): [dict(knobs=dict(BLOCK=64, G=2), path="step", fx="A6", tuning=dict(block=64, ap=0, G=2))],
    (64, 3, 0, 0): [dict(knobs=dict(BLOCK=64, G=4), path="step", fx="A3", tuning=dict(block=64, ap=3, G=4))],
    (64, 10, 0, 0): [dict(knobs=dict(BLOCK=64, G=3), path="step", fx="A10", tuning=dict(block=64, ap=10, G=3))],
    (128, 0, 0, 0): [dict(knobs=dict(BLOCK=128, G=5), path="step", fx="A6", tuning=dict(block=128, ap=0, G=5))],
    (128, 3, 0, 0): [dict(knobs=dict(BLOCK=128, G=7), path="step", fx="A3", tuning=dict(block=128, ap=3, G=7))],
    (128, 10, 0, 0): [dict(knobs=dict(BLOCK=128, G=4), path="step", fx="A10", tuning=dict(block=128, ap=10, G=4))],
    (256, 0, 0, 0): [dict(knobs=dict(BLOCK=256, G=4, AP=0), path="step", fx="A10", tuning=dict(block=256, ap=0, G=4))],
    (256, 3, 0, 0): [dict(knobs=dict(BLOCK=256, G=6), path="step", fx="A3", tuning=dict(block=256, ap=3, G=6))],
    (256, 10, 0, 0): [dict(knobs=dict(BLOCK=256, G=4, NT=1), path="step", fx="A10", tuning=dict(block=256, ap=10, G=4, nt=1)),
                      dict(knobs=dict(BLOCK=256, G=5, SPEC=0), path="step", fx="A10", tuning=dict(block=256, ap=10, G=5, spec=0))],
    (256, 10, 1, 0): [dict(knobs=dict(BLOCK=256, G=3), path="step", fx="A10", tuning=dict(block=256, ap=10, G=3, nt=0, spec=1))],
    (256, 10, 1, 4): [dict(knobs=dict(BLOCK=256, G=4), path="step", fx="A10", tuning=dict(block=256, ap=10, G=4, nt=0, spec=1))],
    (64, 0, 2, 0): [dict(knobs=dict(BLOCK=64, G=3), path="rollout", fx="A10", tuning=dict(block_roll=64, G_roll=3, roll=1))],
    (256, 0, 2, 0): [dict(knobs=dict(GROLL=5), path="rollout", fx="A3", tuning=dict(block_roll=256, ap=3, G_roll=5, roll=1)),
                     dict(knobs=dict(GROLL=4, AP=0), path="step_many", fx="A10", tuning=dict(block_roll=256, ap=0, G_roll=4, roll=1))],
    (256, 10, 2, 0): [dict(knobs=dict(GROLL=3), path="rollout", fx="A10", tuning=dict(block_roll=256, ap=10, G_roll=3, roll=1))],
    (256, 10, 2, 4): [dict(knobs=dict(GROLL=4), path="rollout", fx="A10", tuning=dict(block_roll=256, ap=10, G_roll=4, roll=1))],
    (256, 10, 2, 6): [dict(knobs=dict(GROLL=6), path="rollout", fx="A10", tuning=dict(block_roll=256, ap=10, G_roll=6, roll=1)),
                      dict(knobs=dict(GROLL=6), path="step_many", fx="A10", tuning=dict(block_roll=256, ap=10, G_roll=6, roll=1))],
}
# navigation_graph (SC 0; SC 1 with walls) has no reference rollout: the same rows, reached by the same knobs and paths, are replayed against the
# oracle alone (test_navigation_graph_variant_vs_oracle). Agent counts and world sizes per fixture shape.
NAV_SCEN = {"nav": dict(scenario_name="navigation_graph"), "navwalls": dict(scenario_name="navigation_graph", num_walls=4)}
NAV_SHAPE = {"A10": (10, 4.0), "A3": (3, 2.0), "A6": (6, 3.0)}

CASES = [(scen, key, i) for key, recipes in sorted(VARIANTS.items()) for i in range(len(recipes)) for scen in SCEN]


def _case_id(c):
    scen, (b, ap, fl, gc), i = c
    r = VARIANTS[(b, ap, fl, gc)][i]
    return "%s-B%d-AP%d-FL%d-GC%d-%s%s" % (scen, b, ap, fl, gc, r["path"], "-" + "-".join("%s%s" % kv for kv in sorted(r["knobs"].items())))


NAV_CASES = [(scen, key, i) for key, recipes in sorted(VARIANTS.items()) for i in range(len(recipes)) for scen in NAV_SCEN]


def _knobs(monkeypatch, knobs):
    for k in ("G", "BLOCK", "GROLL", "AP", "NT", "SPEC", "ROLL", "ROLLNT", "SPLIT"):
        monkeypatch.delenv("GMPE_" + k, raising=False)
    monkeypatch.setenv("GMPE_SPLIT", "0")
    for k, v in knobs.items():
        monkeypatch.setenv("GMPE_" + k, str(v))


@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_reference_rollout_through_variant(monkeypatch, case):
    from test_gpu_parity import _engine
    scen, key, i = case
    r = VARIANTS[key][i]
    _knobs(monkeypatch, r["knobs"])
    path = os.path.join(GOLD, FIXTURES[scen][r["fx"]] + ".npz")
    N = _tile_envs(r)
    mb = R.MixedBatch(path, N, R.fixture_slots(N, _tile_G(r)), seed=sum(key) + 17 * i)
    assert mb.guided and mb.d["st_status"].any() and mb.d["st_prev_phase"].max() == 2 and mb.did_reset.any()
    eng = _engine(mb.cfg)
    _assert_tuning(eng, r)
    R.replay_on_gpu(eng, mb, r["path"])
    eng.close()


def _tile_G(r):
    return r["tuning"].get("G_roll" if r["path"] != "step" else "G", 1)


def _tile_envs(r):
    G = _tile_G(r)
    return 4 * G + (G + 1) // 2                                      # five tiles, the last one partial


def _assert_tuning(eng, r):
    t = eng.tuning()
    for f, v in r["tuning"].items():
        assert t[f] == v, (f, t[f], v)
    assert t["split"] == 0


@pytest.mark.parametrize("case", NAV_CASES, ids=[_case_id(c) for c in NAV_CASES])
def test_navigation_graph_variant_vs_oracle(monkeypatch, case):
    """navigation_graph's instantiations (SC 0, and SC 1 with walls), row by row of VARIANTS with the row's knobs and launch path: every env
    against the oracle every step (segment ends on step_many), masks on the rollout path, resets inside the kernel under test."""
    from test_gpu_parity import _engine
    scen, key, i = case
    r = VARIANTS[key][i]
    _knobs(monkeypatch, r["knobs"])
    A, ws = NAV_SHAPE[r["fx"]]
    cfg = gmpe.make_config(num_envs=_tile_envs(r), num_agents=A, world_size=ws, episode_length=9, seed=400 + sum(key) + 17 * i, **NAV_SCEN[scen])
    eng = _engine(cfg)
    _assert_tuning(eng, r)
    n_resets = R.replay_on_gpu(eng, R.OracleBatch(cfg, T=24, seg=8, seed=i), r["path"])
    assert n_resets >= 2 * cfg.num_envs
    eng.close()


# ---------------------------------------------------------------- bit-identity between instantiations of one scenario
# Tile shape, rollout vs step loop, nontemporal stores and wave specialisation must not change a bit (the suite's standing claim): every
# exact-size row (AP = 10) is compared with the first one, every run-time-size row (AP = 0) with the first of those, for one mixed batch.
# Exact-size vs run-time-size outputs (AP = 10 vs AP = 0), asserted nowhere before: measured bit-identical on MI355X for all four tube scenarios
# (every output of every step and the final state), and held to that.
IDENT_N = 27


def _ident_recipes():
    out = {10: [], 0: []}
    for key, recipes in sorted(VARIANTS.items()):
        for r in recipes:
            if r["fx"] == "A10":
                out[key[1]].append((key, r))
    return out


@pytest.mark.parametrize("scen", SCEN)
def test_instantiations_are_bit_identical(monkeypatch, scen):
    import numpy as np
    import torch
    from test_gpu_parity import _engine
    path = os.path.join(GOLD, FIXTURES[scen]["A10"] + ".npz")
    runs = {}
    for ap, recipes in _ident_recipes().items():
        assert len(recipes) >= 3
        for key, r in recipes:
            _knobs(monkeypatch, r["knobs"])
            mb = R.MixedBatch(path, IDENT_N, R.fixture_slots(IDENT_N, 4), seed=5)
            eng = _engine(mb.cfg)
            _assert_tuning(eng, r)
            runs.setdefault(ap, []).append(((key, r["path"], tuple(sorted(r["knobs"].items()))),) + R.run_outputs(eng, mb, "step" if r["path"] == "step" else "rollout"))
            eng.close()
    for ap, rs in runs.items():
        (lab0, st0, s0) = rs[0]
        for lab, st, s in rs[1:]:
            for k in R.OUT_KEYS:
                assert torch.equal(st[k], st0[k]), (ap, lab, lab0, k)
            for f in s0:
                np.testing.assert_array_equal(s[f], s0[f], err_msg="%s vs %s: %s" % (lab, lab0, f))
    (lab_a, a, sa), (lab_b, b, sb) = runs[10][0], runs[0][0]
    for k in R.OUT_KEYS:
        assert torch.equal(a[k], b[k]), ("AP10 vs AP0", lab_a, lab_b, k, float((a[k].double() - b[k].double()).abs().max()))
    for f in sa:
        np.testing.assert_array_equal(sa[f], sb[f], err_msg="AP10 vs AP0 state " + f)


# ---------------------------------------------------------------- the bench launches with reference envs inside
BENCH_FIXTURES = {"c3": "july_A10_s0", "c3r": "rotinv_A10_s8", "c3p2": "twophase_A10_s22", "c3p3": "threephase_A10_s42"}


def _bench_batch(workload):
    mb = R.MixedBatch(os.path.join(GOLD, BENCH_FIXTURES[workload] + ".npz"), 4096, R.spread_slots(4096, 8), seed=7)
    c = mb.cfg
    assert (c.num_agents, c.world_size, c.episode_length, c.num_obstacles) == (10, 4.0, 25, 0) and 4095 in mb.slots and len(mb.slots) == 8
    return mb


@pytest.mark.parametrize("workload", sorted(BENCH_FIXTURES))
def test_bench_rollout_launch_with_reference_envs(monkeypatch, workload):
    """The launch _bench_shape_rollout reproduces: the auto-chosen tile (exact size, G_roll = 6: k_env<256, 10, SC, 2, 6>), one rollout into 26 slots
    past the Infinity Cache (nontemporal stores), no masks, the slots wrapping. The fixture slots against the reference in every surviving slot,
    all 4096 envs against the oracle."""
    import torch
    from gmpe.engine import StepOutputs
    import oracle_lib as ol
    from test_gpu_parity import _engine
    _knobs(monkeypatch, {})
    monkeypatch.delenv("GMPE_SPLIT")
    mb = _bench_batch(workload)
    eng, orc = _engine(mb.cfg), ol.Oracle(mb.cfg)
    t = eng.tuning()
    assert t["ap"] == 10 and t["G_roll"] == 6 and t["block_roll"] == 256 and t["roll"] == 1 and t["split"] == 0
    mb.start(eng, orc)
    K, n_slots = mb.T, 26
    assert K > n_slots
    o = eng.out
    slots = {k: torch.empty((n_slots,) + tuple(getattr(o, k).shape), dtype=getattr(o, k).dtype, device="cuda") for k in R.OUT_KEYS}
    step_bytes = sum(getattr(o, k).numel() * getattr(o, k).element_size() for k in R.OUT_KEYS)
    assert step_bytes * n_slots > (256 << 20)
    acts = torch.as_tensor(mb.acts, device="cuda")
    eng.rollout(acts, K, slot0=StepOutputs(**{k: v[0] for k, v in slots.items()}), num_slots=n_slots, strides={k: v[0].numel() for k, v in slots.items()})
    torch.cuda.synchronize()
    n_checked = 0
    for k in range(K):
        oo = orc.step(mb.acts[k])
        if k < K - n_slots:
            continue
        view = {key: v[k % n_slots] for key, v in slots.items()}
        mb.check_outputs(R._outputs(view), k, "bench slot %d" % (k % n_slots))
        R._oracle_step(R._View(**view), oo, mb.cfg, "bench step %d" % k)
        n_checked += 1
    assert n_checked == n_slots and mb.did_reset[:K].any()
    assert not mb.did_reset[K - 1]
    mb.check_state(eng, K - 1, "bench end")
    R._oracle_state(eng, orc, "bench end")
    assert not eng.get("error_flags").any()
    eng.check_errors()
    eng.close()


@pytest.mark.parametrize("workload", sorted(BENCH_FIXTURES))
def test_bench_step_loop_with_reference_envs(monkeypatch, workload):
    """The same batch through the steady-state step kernel (FL = 1, the closed-loop shape: k_env<256, 10, SC, 1, 4> at G = 4; two_phase, whose GC = 4
    step kernel is compiled for three waves per SIMD, is resident at G = 6 and runs k_env<256, 10, SC_TWO, 1>), one step() per step: fixture slots
    against the reference every step, reset steps' placement included, all 4096 envs against the oracle every step."""
    from test_gpu_parity import _engine
    _knobs(monkeypatch, {})
    monkeypatch.delenv("GMPE_SPLIT")
    mb = _bench_batch(workload)
    eng = _engine(mb.cfg)
    t = eng.tuning()
    assert t["ap"] == 10 and t["G"] == (6 if workload == "c3p2" else 4) and t["block"] == 256 and t["nt"] == 0 and t["spec"] == 1 and t["split"] == 0
    n_resets = R.replay_on_gpu(eng, mb, "step")
    assert n_resets >= 4096
    eng.close()
