"""CPU side of the batched evaluator (include/gmpe.h gmpe_episode_record / _metrics / _summary, gmpe.evaluate): the NumPy restatement
(tests/eval_lib.py) against the reference's own render loop (tests/golden/eval_metrics.npz), the summary labels and csv row order, the plan
layouts and the C entry points' argument checks (refused before any device call)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import abi_lib  # noqa: E402
import eval_lib as EL  # noqa: E402
from gmpe import _lib  # noqa: E402
from gmpe import evaluate as EV  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")
FIX = np.load(os.path.join(GOLDEN, "eval_metrics.npz"))
ROLLOUTS = [str(r) for r in FIX["rollouts"]]
DT, THRESH = float(FIX["dt"]), float(FIX["min_dist_thresh"])


def _replay(name):
    """Every episode of the rollout through eval_lib.Record (one env each, the recorded f64 rows), then the columns."""
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    A, T = int(d["A"]), int(d["episode_length"])
    segs = EL.cut_episodes(np.asarray(d["did_reset"], bool), T)
    W = d["info"].shape[-1]
    fi, ret, steps = np.zeros((len(segs), A, W)), np.zeros((len(segs), A)), np.zeros(len(segs), np.int32)
    for i, (s, n) in enumerate(segs):
        rec = EL.Record(1, A, T, width=W, dtype=np.float64)
        for t in range(n):
            rec.step(d["rew"][s + t][None], d["done"][s + t][None], d["info"][s + t][None])
        assert rec.steps[0] == n and not rec.live[0]
        fi[i], ret[i], steps[i] = rec.final_info[0], rec.ret[0], rec.steps[0]
    return d, A, T, segs, fi, ret, steps


@pytest.mark.parametrize("name", ROLLOUTS)
def test_numpy_restatement_is_the_reference_render_loop(name):
    d, A, T, segs, fi, ret, steps = _replay(name)
    np.testing.assert_array_equal(np.array(segs), FIX[name + "/seg"])
    cols = EL.episode_columns(fi, ret, steps, T, DT, THRESH)
    np.testing.assert_array_equal(cols, FIX[name + "/cols"])
    np.testing.assert_array_equal(cols[:, EL.COLUMNS.index("success")], FIX[name + "/success_a"].mean(axis=1))
    dists, times = EL.agent_sums(fi, T, DT)
    np.testing.assert_allclose(dists, FIX[name + "/dists_trav"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(times, FIX[name + "/time_taken"], rtol=1e-12, atol=0)
    # the summary under the reference's own labels, in the order it prints them
    summ = EV.summary_from_stats(EL.summary_stats(cols, A), dists, times, len(segs))
    labels = [str(x) for x in FIX[name + "/labels"]]
    assert labels == [lab for lab, _, _ in EV.SUMMARY_LABELS]
    np.testing.assert_array_equal(np.array([summ[lab] for lab in labels]), FIX[name + "/values"])
    # csv_data: its order and values, the per-agent lists in place
    row = EV.csv_values(summ, A, T, 0, float(d["world_size"]))
    lens = [np.atleast_1d(v).size for v in row]
    np.testing.assert_array_equal(lens, FIX[name + "/csv_lens"])
    flat = np.concatenate([np.atleast_1d(np.asarray(v, np.float64)) for v in row])
    np.testing.assert_allclose(flat, FIX[name + "/csv"], rtol=1e-12, atol=0)


def test_fixture_covers_every_family_and_early_ends():
    for fam in ("july", "rotinv", "twophase", "threephase"):
        assert any(n.startswith(fam) for n in ROLLOUTS), fam
    lengths = np.concatenate([FIX[n + "/seg"][:, 1] for n in ROLLOUTS])
    Ts = np.concatenate([np.full(len(FIX[n + "/seg"]), int(FIX[n + "/T"])) for n in ROLLOUTS])
    assert (lengths < Ts).any() and (lengths == Ts).any()        # episodes cut by the all-done break and by the end of the range


def test_record_restatement_masks_and_stop_rows():
    rec = EL.Record(3, 2, 4, n_actions=5)
    done = np.array([[1, 0], [1, 1], [0, 0]], bool)
    masks, avail = rec.step(np.ones((3, 2), np.float32), done, np.zeros((3, 2, 18), np.float32))
    np.testing.assert_array_equal(masks[..., 0], [[0, 1], [1, 1], [1, 1]])
    np.testing.assert_array_equal(avail[0, 0], [0, 0, 1, 0, 0])
    assert (avail[0, 1] == 1).all() and (avail[1:] == 1).all()
    assert list(rec.live) == [True, False, True] and list(rec.steps) == [0, 1, 0]


def test_new_symbols_are_exported_and_bound():
    assert {"gmpe_episode_record", "gmpe_episode_metrics", "gmpe_episode_summary"} <= set(_lib.SYMBOLS) & abi_lib.exported()


def test_plan_layouts_match_the_c_header():
    """The three plans in the numbers they were designed with, read from the header (that the mirror has them too is tests/test_abi_host.py's)."""
    (r, R), (m, Mp), (s, S) = (abi_lib.layout(P) for P in (_lib.GmpeEpisodeRecordPlan, _lib.GmpeEpisodeMetricsPlan, _lib.GmpeEpisodeSummaryPlan))
    assert r == 6 * 4 + 10 * 8 and R["reward"][0] == 24 and R["rnn_states"][0] == 24 + 9 * 8
    assert m == 16 + 16 + 6 * 8 and Mp["dt"][0] == 16 and Mp["steps"][0] == 32 and Mp["time_taken"][0] == 72
    assert s == 8 + 16 + 16 and S["table"][0] == 24 and S["out"][0] == 32
    assert _lib.EVAL_NUM_COLUMNS == len(EV.COLUMNS) == len(EL.COLUMNS) and EV.COLUMNS == EL.COLUMNS
    assert _lib.EVAL_NUM_STATS == len(EV.STATS) and _lib.EVAL_INFO_WIDTH == len(EL.KEYS)
    from gmpe.config import INFO_KEYS
    assert EL.KEYS == INFO_KEYS
    assert "#define GMPE_ABI_VERSION 3" in open(abi_lib.HDR).read()


FAKE = 0x1000      # an aligned non-null address: every plan below is refused before it could be used


def _record(**kw):
    p = _lib.GmpeEpisodeRecordPlan()
    p.num_envs, p.num_agents, p.t, p.num_steps, p.n_actions = 8, 3, 0, 5, 25
    for f in ("reward", "done", "info", "live", "steps", "ret", "final_info", "masks", "available_actions"):
        setattr(p, f, FAKE)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _metrics(**kw):
    p = _lib.GmpeEpisodeMetricsPlan()
    p.num_envs, p.num_agents, p.num_steps, p.dt, p.min_dist_thresh = 8, 3, 5, 1.0, 0.05
    for f in ("steps", "ret", "final_info", "episodes", "dists_traveled", "time_taken"):
        setattr(p, f, FAKE)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _summary(**kw):
    p = _lib.GmpeEpisodeSummaryPlan()
    p.num_rows, p.num_columns, p.success_column, p.success_agents, p.table, p.out = 100, 16, 2, 3, FAKE, FAKE
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("fn, plan, msg", [
    ("gmpe_episode_record", _record(t=5), "0 <= t < num_steps"),
    ("gmpe_episode_record", _record(t=-1), "0 <= t < num_steps"),
    ("gmpe_episode_record", _record(num_steps=0, t=0), "num_steps >= 1"),
    ("gmpe_episode_record", _record(num_envs=0), "num_envs >= 1"),
    ("gmpe_episode_record", _record(num_agents=65), "num_agents <= 64"),
    ("gmpe_episode_record", _record(n_actions=0), "n_actions"),
    ("gmpe_episode_record", _record(reward=None), "null pointer"),
    ("gmpe_episode_record", _record(info=None), "null pointer"),
    ("gmpe_episode_record", _record(live=None), "null pointer"),
    ("gmpe_episode_record", _record(masks=None), "null pointer"),
    ("gmpe_episode_record", _record(available_actions=None), "null pointer"),
    ("gmpe_episode_record", _record(rnn_states=FAKE, rnn_row=0), "rnn_row"),
    ("gmpe_episode_record", _record(ret=FAKE + 4), "misaligned"),
    ("gmpe_episode_record", _record(masks=FAKE + 2), "misaligned"),
    ("gmpe_episode_metrics", _metrics(num_steps=0), "num_steps >= 1"),
    ("gmpe_episode_metrics", _metrics(dt=0.0), "dt"),
    ("gmpe_episode_metrics", _metrics(dt=float("nan")), "dt"),
    ("gmpe_episode_metrics", _metrics(reserved=1), "reserved"),
    ("gmpe_episode_metrics", _metrics(episodes=None), "null pointer"),
    ("gmpe_episode_metrics", _metrics(time_taken=None), "together"),
    ("gmpe_episode_metrics", _metrics(num_agents=0), "num_agents"),
    ("gmpe_episode_metrics", _metrics(ret=FAKE + 4), "misaligned"),
    ("gmpe_episode_summary", _summary(num_rows=0), "num_rows"),
    ("gmpe_episode_summary", _summary(num_rows=1 << 31), "num_rows"),
    ("gmpe_episode_summary", _summary(num_columns=65), "num_columns"),
    ("gmpe_episode_summary", _summary(success_column=16), "success_column"),
    ("gmpe_episode_summary", _summary(success_agents=0), "success_agents"),
    ("gmpe_episode_summary", _summary(table=None), "null pointer"),
    ("gmpe_episode_summary", _summary(out=FAKE + 4), "misaligned"),
])
def test_c_side_refuses_bad_plans_before_any_device_call(fn, plan, msg):
    lib = _lib.load()
    assert getattr(lib, fn)(0, C.byref(plan), None) == -1                         # GMPE_ERR_INVALID_ARG
    err = lib.gmpe_last_error()
    assert err.startswith(fn.encode() + b": ") and msg.encode() in err, err


@pytest.mark.parametrize("fn", ["gmpe_episode_record", "gmpe_episode_metrics", "gmpe_episode_summary"])
def test_c_side_null_plan(fn):
    lib = _lib.load()
    assert getattr(lib, fn)(0, None, None) == -1 and b"null plan" in lib.gmpe_last_error()


def test_python_layer_refuses_what_is_not_an_engine():
    with pytest.raises(TypeError, match="GmpeEngine"):
        EV.BatchedEvaluator(object())
    with pytest.raises(TypeError, match="GmpeEngine"):
        EV.evaluate(object(), lambda *a: None)


def test_summary_labels_and_csv_order():
    labels = [lab for lab, _, _ in EV.SUMMARY_LABELS]
    assert len(labels) == len(set(labels)) == 54
    assert labels[:3] == ["Rewards", "Frac of episode", "Success rates mean"] and "Fair 0.9 Quantile:" in labels
    stats = {c: {k: float(10 * i + j) for j, k in enumerate(EV.STATS)} for i, c in enumerate(EV.COLUMNS)}
    s = EV.summary_from_stats(stats, [1.0, 2.0], [3.0, 4.0], 7)
    row = EV.csv_values(s, 2, 5, 3, 4.0)
    assert row[:5] == [3, 2, 4.0, 5, 7]
    assert len(row) == 69 and row[5] == stats["frac"]["mean"] and row[-1] == stats["spacing_violations"]["std"]
    np.testing.assert_array_equal(row[16], [1.0, 2.0])
    np.testing.assert_array_equal(row[17], [3.0, 4.0])
    assert row[13] == stats["reward"]["mean"] and row[14] == stats["reward"]["mean"] / 2 and row[15] == stats["reward"]["mean"] / 10
