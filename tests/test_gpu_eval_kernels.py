"""The three evaluation kernels (csrc/gmpe_eval.hip) driven directly through their handle-less C entry points on synthetic tensors, at the
shapes and values an engine never produces (inputs, exact references and the derived bounds: tests/eval_lib.py; the inputs are proven sharp
on the CPU in tests/test_eval_kernel_inputs_host.py).

1. gmpe_episode_summary: every input family of eval_lib.summary_columns at 19 row counts and 1 / 5 / 16 / 64 columns. Order statistics equal to
   NumPy's (zeros by value); mean and std within the derived bounds of exact rational arithmetic, and within 1e-12 of NumPy where both must be.
2. gmpe_episode_metrics: 14 agent counts x 5 env counts, the columns equal to float64 NumPy, the sums over agents against math.fsum as well.
3. gmpe_episode_record: step by step against eval_lib.Record, everything exact, the RNN rows against a ramp.
"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import eval_lib as EL  # noqa: E402
from gmpe import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 0


def _dev(a):
    return torch.from_numpy(np.array(a)).to("cuda:%d" % DEV)           # a writable, contiguous copy: the inputs are read-only


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


# ------------------------------------------------------------------------------------------------------------------------------ summary

_SUMMARY = {}


def _summary(n, ti):
    """f64 [C, 7] of table ti at n rows, computed once. The output starts as -7.0: a statistic the kernel does not write shows."""
    if (n, ti) not in _SUMMARY:
        t = EL.summary_tables(n)[ti]
        tab = _dev(t["table"])
        out = torch.full((tab.shape[1], _lib.EVAL_NUM_STATS), -7.0, dtype=torch.float64, device=tab.device)
        sp = _lib.GmpeEpisodeSummaryPlan()
        sp.num_rows, sp.num_columns, sp.success_column, sp.success_agents = n, tab.shape[1], t["success_column"], t["success_agents"]
        sp.table, sp.out = tab.data_ptr(), out.data_ptr()
        _lib.check(_lib.load().gmpe_episode_summary(DEV, C.byref(sp), _stream()), "gmpe_episode_summary")
        _SUMMARY[(n, ti)] = out.cpu().numpy()
    return _SUMMARY[(n, ti)]


def _same(a, b):
    return a == b or (a != a and b != b)          # -0.0 == +0.0: the sign of a zero is not pinned (NumPy's sort does not order them)


@pytest.mark.parametrize("n,ti,ci,name", EL.summary_cases(), ids=lambda v: str(v))
def test_summary_column(n, ti, ci, name):
    t = EL.summary_tables(n)[ti]
    x = t["table"][:, ci]
    got = dict(zip(EL.STATS, _summary(n, ti)[ci].tolist()))
    label = "n=%d C=%d column %d (%s)" % (n, t["table"].shape[1], ci, name)
    if name.startswith("succ."):
        A = t["success_agents"]
        ref = EL.success_flat_stats(x, A)
        S, total = int(np.rint(x * A).sum()), n * A
        p = S / total                                                    # exact: one division of two integers below 2^53
        exact = {"mean": p, "std": math.sqrt((total - S) * S) / total}   # sqrt(p (1 - p)) with one rounding in the root and one in the division
        print(label, got, ref)
        for k in EL.ORDER_STATS:
            assert _same(got[k], float(ref[k])), "%s %s: %r vs %r" % (label, k, got[k], ref[k])
        assert got["mean"] == exact["mean"], "%s mean: %r vs %r" % (label, got["mean"], exact["mean"])
        # the kernel's closed form has five roundings on well-scaled terms (p^2, (1-p)^2, two products, a sum of non-negatives), a division
        # and a root: 8 u relative at most, next to 2 u in the reference
        assert abs(got["std"] - exact["std"]) <= 10 * 2.0 ** -53 * exact["std"], "%s std: %r vs %r" % (label, got["std"], exact["std"])
        np.testing.assert_allclose([got["mean"], got["std"]], [ref["mean"], ref["std"]], rtol=1e-12, atol=1e-300, err_msg=label)
        return
    ref = EL.quiet(EL.stats_of, x)
    print(label, got, ref)
    for k in EL.ORDER_STATS:
        assert _same(got[k], float(ref[k])), "%s %s: %r vs %r" % (label, k, got[k], ref[k])
    if name.startswith("nan@"):
        assert all(v != v for v in got.values()), "%s: %r" % (label, got)
    if EL.is_normal_finite(x):
        mom = EL.exact_moments(x)
        print(label, "mean error, std error, std bound:", EL.check_mean_std(x, got["mean"], got["std"], mom))
        mean_ok, std_ok = EL.numpy_agreement(x, mom)
        if mean_ok:
            np.testing.assert_allclose(got["mean"], ref["mean"], rtol=1e-12, atol=0, err_msg=label + " mean")
        if std_ok:
            np.testing.assert_allclose(got["std"], ref["std"], rtol=1e-12, atol=0, err_msg=label + " std")
    else:                                                                # subnormal, inf, NaN: NumPy's own result
        np.testing.assert_allclose([got["mean"], got["std"]], [ref["mean"], ref["std"]], rtol=1e-12, atol=0, equal_nan=True, err_msg=label)


# ------------------------------------------------------------------------------------------------------------------------------ metrics

def _metrics(fi, ret, steps, sums=True):
    N, A = ret.shape
    d_fi, d_ret, d_steps = _dev(fi), _dev(ret), _dev(steps)
    rows = torch.full((N, _lib.EVAL_NUM_COLUMNS), -7.0, dtype=torch.float64, device=d_fi.device)
    agent = torch.full((2, A), -7.0, dtype=torch.float64, device=d_fi.device)
    mp = _lib.GmpeEpisodeMetricsPlan()
    mp.num_envs, mp.num_agents, mp.num_steps, mp.dt, mp.min_dist_thresh = N, A, EL.METRIC_T, EL.METRIC_DT, EL.METRIC_THRESH
    mp.steps, mp.ret, mp.final_info, mp.episodes = d_steps.data_ptr(), d_ret.data_ptr(), d_fi.data_ptr(), rows.data_ptr()
    if sums:
        mp.dists_traveled, mp.time_taken = agent[0].data_ptr(), agent[1].data_ptr()
    _lib.check(_lib.load().gmpe_episode_metrics(DEV, C.byref(mp), _stream()), "gmpe_episode_metrics")
    return rows.cpu().numpy(), agent.cpu().numpy()


@pytest.mark.parametrize("N", EL.METRIC_ENVS)
@pytest.mark.parametrize("A", EL.METRIC_AGENTS)
def test_metrics(A, N):
    fi, ret, steps = EL.metrics_inputs(N, A)
    rows, agent = _metrics(fi, ret, steps)
    ref = EL.quiet(EL.episode_columns, fi, ret, steps, EL.METRIC_T, EL.METRIC_DT, EL.METRIC_THRESH)
    np.testing.assert_array_equal(rows, ref, err_msg="A=%d N=%d episode columns vs float64 NumPy" % (A, N))
    col = {c: rows[:, i] for i, c in enumerate(EL.COLUMNS)}
    # the Time_req_to_goal patterns, stated without NumPy's reductions
    tdt = EL.METRIC_T * EL.METRIC_DT
    for i in range(N):
        p = EL.row_pattern(i, A)
        if p.startswith("nan"):
            assert np.isnan(col["frac"][i]) and np.isnan(col["total_time_taken"][i]), "A=%d row %d (%s)" % (A, i, p)
        elif p == "all -1":
            assert col["frac"][i] == 1.0 and col["total_time_taken"][i] == EL.kernel_np_sum([tdt] * A), "A=%d row %d (%s)" % (A, i, p)
        else:
            assert col["frac"][i] == col["frac"][i], "A=%d row %d (%s)" % (A, i, p)
    d2g = fi[..., EL.K["Dist_to_goal"]]
    np.testing.assert_array_equal(col["success"], (d2g < np.float32(EL.METRIC_THRESH)).sum(1) / A)      # at the threshold: not a success
    assert (d2g == np.float32(EL.METRIC_THRESH)).any()
    # second, independent reference of the sums over agents: exact arithmetic, any summation order
    f64 = fi.astype(np.float64)
    ttg = np.where(f64[..., EL.K["Time_req_to_goal"]] == -1, tdt, f64[..., EL.K["Time_req_to_goal"]])
    EL.check_sums(col["reward"], ret, A, "reward")
    EL.check_sums(col["total_time_taken"], ttg, 1, "total_time_taken")
    for c, key, mean in EL.SUMMED:
        EL.check_sums(col[c], f64[..., EL.K[key]], A if mean else 1, c)
    # per-agent sums over the episodes
    ref_d, ref_t = EL.agent_sums(fi, EL.METRIC_T, EL.METRIC_DT)
    EL.check_sums(agent[0], f64[..., EL.K["Dists_traveled"]].T, 1, "dists_traveled")
    EL.check_sums(agent[1], ttg.T, 1, "time_taken")
    for x in (f64[..., EL.K["Dists_traveled"]], np.nan_to_num(ttg)):
        assert (N * 2.0 ** -53 * np.abs(x).sum(0) <= 0.5e-12 * np.abs(x.sum(0))).all()       # where NumPy and the kernel must meet within 1e-12
    np.testing.assert_allclose(agent[0], ref_d, rtol=1e-12, atol=0)
    np.testing.assert_allclose(agent[1], ref_t, rtol=1e-12, atol=0, equal_nan=True)
    # without the per-agent sums: no extra workgroups, the same table
    rows2, agent2 = _metrics(fi, ret, steps, sums=False)
    np.testing.assert_array_equal(rows2, rows)
    assert (agent2 == -7.0).all()


# ------------------------------------------------------------------------------------------------------------------------------ record

def _ramp(shape, device):
    """A sentinel that is neither 0 nor 1 and differs from row to row: a write to the wrong row shows."""
    n = int(np.prod(shape))
    return (torch.arange(n, device=device, dtype=torch.int64) % 8191 + 2).to(torch.float32).reshape(shape)


def _run_record(N, A, na, rnn_row, T, seed, pattern=None):
    rew, done, info = EL.record_inputs(N, A, T, seed, pattern)
    dev = torch.device("cuda:%d" % DEV)
    live = torch.ones((N,), dtype=torch.uint8, device=dev)
    steps = torch.zeros((N,), dtype=torch.int32, device=dev)
    ret = torch.zeros((N, A), dtype=torch.float64, device=dev)
    final = torch.zeros((N, A, _lib.EVAL_INFO_WIDTH), dtype=torch.float32, device=dev)
    masks = torch.full((N, A, 1), -7.0, dtype=torch.float32, device=dev)
    avail = torch.full((N, A, na), -7.0, dtype=torch.float32, device=dev)
    rnn = ramp = None
    if rnn_row is not None:
        ramp = _ramp((N, A, rnn_row), dev)
        rnn = torch.empty_like(ramp)
    rp = _lib.GmpeEpisodeRecordPlan()
    rp.num_envs, rp.num_agents, rp.num_steps, rp.n_actions = N, A, T, na
    rp.live, rp.steps, rp.ret, rp.final_info = live.data_ptr(), steps.data_ptr(), ret.data_ptr(), final.data_ptr()
    rp.masks, rp.available_actions = masks.data_ptr(), avail.data_ptr()
    if rnn is not None:
        rp.rnn_states, rp.rnn_row = rnn.data_ptr(), rnn_row
    rec = EL.Record(N, A, T, n_actions=na)
    label = "N=%d A=%d n_actions=%d rnn_row=%r T=%d" % (N, A, na, rnn_row, T)
    for t in range(T):
        d_rew, d_done, d_info = _dev(rew[t]), _dev(done[t].astype(np.uint8)), _dev(info[t])
        if rnn is not None:
            rnn.copy_(ramp)
        rp.t = t
        rp.reward, rp.done, rp.info = d_rew.data_ptr(), d_done.data_ptr(), d_info.data_ptr()
        _lib.check(_lib.load().gmpe_episode_record(DEV, C.byref(rp), _stream()), "gmpe_episode_record")
        m, av = rec.step(rew[t], done[t], info[t])
        np.testing.assert_array_equal(masks.cpu().numpy(), m, err_msg="%s t=%d masks" % (label, t))
        np.testing.assert_array_equal(avail.cpu().numpy(), av, err_msg="%s t=%d available_actions" % (label, t))
        all_done = done[t].all(axis=1)
        assert (m[all_done] == 1.0).all()
        if rnn is not None:               # zero where done, the ramp elsewhere; compared on the device (a row can be 2^16 floats wide)
            want = torch.where(d_done.bool()[..., None], torch.zeros((), device=dev), ramp)
            assert torch.equal(rnn, want), "%s t=%d rnn rows: %d elements differ" % (label, t, int((rnn != want).sum()))
    np.testing.assert_array_equal(live.cpu().numpy().astype(bool), rec.live, err_msg=label + " live")
    assert not rec.live.any()
    np.testing.assert_array_equal(steps.cpu().numpy(), rec.steps, err_msg=label + " steps")
    np.testing.assert_array_equal(ret.cpu().numpy(), rec.ret, err_msg=label + " ret")
    np.testing.assert_array_equal(final.cpu().numpy().view(np.int32), rec.final_info.view(np.int32), err_msg=label + " final_info bits")
    return rec, done


@pytest.mark.parametrize("N,A,na,rnn_row,T", EL.record_cases())
def test_record(N, A, na, rnn_row, T):
    _run_record(N, A, na, rnn_row, T, seed=N + A + na + T)


@pytest.mark.parametrize("T", EL.RECORD_STEPS)
@pytest.mark.parametrize("pattern", EL.DONE_PATTERNS)
def test_record_done_pattern(pattern, T):
    N, A = 33, 5
    rec, done = _run_record(N, A, 25, 7, T, seed=T, pattern=pattern)
    all_done = done.all(axis=2)                                   # [T, N]
    first = np.where(all_done.any(0), all_done.argmax(0), T - 1)
    np.testing.assert_array_equal(rec.steps, first + 1)
    if pattern == "finished at step 0":
        assert (rec.steps == 1).all()
    if pattern in ("never", "only by the last step"):
        assert (rec.steps == T).all() and not all_done.any()


def test_record_rnn_row_65536():
    N, A, row = 16, 64, 1 << 16
    try:
        torch.empty((3, N, A, row), dtype=torch.float32, device="cuda:%d" % DEV)
    except RuntimeError as e:                                     # 3 x 268 MB: the states, the ramp and the expected tensor
        pytest.skip("cannot allocate the 268 MB rnn_states tensors: %s" % e)
    _run_record(N, A, 25, row, 2, seed=9)
