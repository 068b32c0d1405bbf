"""The synthetic inputs of tests/test_gpu_eval_kernels.py are sharp: each cheap wrong variant of the reference disagrees with the true reference
on them, so a kernel with that mistake cannot pass. CPU only. The conditions here are conditions on the inputs, not tolerances on a kernel."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import eval_lib as EL  # noqa: E402

NS = [n for n in EL.SUMMARY_NS if n > 1]
FAMILIES = ["randn", "lowbytes", "f32w"]


def _gamma_tenths(n, q):
    v = (n - 1) * (q / 100.0)
    return v - math.floor(v)


def test_gamma_table_covers_both_lerp_halves():
    for n in EL.SUMMARY_NS:
        g10, g90 = _gamma_tenths(n, 10.0), _gamma_tenths(n, 90.0)
        t = EL.GAMMA_P10_TENTHS[n]
        assert abs(g10 - t / 10.0) < 1e-9 and abs(g90 - ((10 - t) % 10) / 10.0) < 1e-9, (n, g10, g90)
    assert sorted(set(EL.GAMMA_P10_TENTHS.values())) == [0, 1, 2, 3, 4, 5, 6, 7, 9]
    exact_zero = [n for n in EL.SUMMARY_NS if _gamma_tenths(n, 10.0) == 0.0]
    assert exact_zero == [1, 11, 101], exact_zero                 # gamma exactly 0, not a rounding away from it
    assert all(_gamma_tenths(n, 90.0) == 0.0 for n in exact_zero)
    below = [n for n in EL.SUMMARY_NS if 0 < _gamma_tenths(n, 10.0) < 0.5]
    above = [n for n in EL.SUMMARY_NS if _gamma_tenths(n, 10.0) >= 0.5]
    assert below and above and 16 in above and 256 in above       # `a + diff * t`, `b - diff * (1 - t)`, and t == 0.5 exactly
    assert _gamma_tenths(16, 10.0) == 0.5 and _gamma_tenths(4096, 10.0) == 0.5
    # lo == hi: only with one row
    assert (1 - 1) * 0.1 >= 1 - 1 and all((n - 1) * 0.9 < n - 1 for n in NS)
    assert {n % 2 for n in EL.SUMMARY_NS} == {0, 1} and {EL.width_of(n) for n in EL.SUMMARY_NS} == {1, 5, 16, 64}
    assert EL.width_of(100003) == 16


def test_every_family_is_present_at_every_row_count():
    for n in EL.SUMMARY_NS:
        names = [m for m, _ in EL.summary_columns(n)]
        want = ["randn", "lowbyte", "lowbyte.neg", "lowbytes", "ties3", "equal", "zeros", "subnormal", "large", "inf1", "f32w", "f32w.pos", "kA"]
        want += ["inf2"] * (n >= 2) + ["nan@%d" % r for r in {0, 255, 256, n - 1} if r < n]
        assert set(want) <= set(names) and len(set(names)) == len(names), (n, names)
        tabs = EL.summary_tables(n)
        assert all(t["table"].shape == (n, EL.width_of(n)) for t in tabs)
        succ = [t for t in tabs if t["success_column"] >= 0]
        assert sorted(t["success_agents"] for t in succ[:4]) == [1, 3, 10, 64] and len(succ) == 6
    cases = EL.summary_cases()
    ids = [c[3] for c in cases]
    for A in EL.SUCCESS_AGENTS:
        for pos in ("first", "mid", "last"):
            assert "succ.A%d@%s" % (A, pos) in ids
    assert any(i.endswith(".zero") for i in ids) and any(i.endswith(".one") for i in ids)
    # n * A odd and even among the success columns
    par = {(c[0] * EL.summary_tables(c[0])[c[1]]["success_agents"]) % 2 for c in cases if c[3].startswith("succ.")}
    assert par == {0, 1}


def test_family_properties():
    for n in EL.SUMMARY_NS:
        d = dict(EL.summary_columns(n))
        # family 1: every byte of the key discriminates somewhere, both signs (n >= 16)
        if n >= 16:
            assert (d["randn"] < 0).any() and (d["randn"] > 0).any()
        # family 2: one shared 7-byte prefix; the spaced distinct variant needs low_bytes_needed(n) bytes
        for k in ("lowbyte", "lowbyte.neg"):
            b = d[k].view(np.uint64)
            assert len(set((b >> np.uint64(8)).tolist())) == 1 and len(set(b.tolist())) == min(n, 256)
        b = d["lowbytes"].view(np.uint64)
        assert len(set((b >> np.uint64(8 * EL.low_bytes_needed(n))).tolist())) == 1 and len(set(b.tolist())) == n
        assert n == 1 or np.diff(np.sort(b).astype(np.int64)).min() >= 13
        assert len(set(d["ties3"].tolist())) <= 3 and len(set(d["equal"].tolist())) == 1
        # family 4: both zeros present from 8 rows on, every inner rank on a zero
        z = d["zeros"]
        if n >= 8:
            assert (np.signbit(z) & (z == 0)).any() and (~np.signbit(z) & (z == 0)).any()
        s = np.sort(z)
        assert all(s[r] == 0 for r in (int((n - 1) * 0.1), min(int((n - 1) * 0.1) + 1, n - 1), n // 2, int((n - 1) * 0.9)))
        if n >= 24:
            assert s[0] < 0 < s[-1]
        tiny = np.finfo(np.float64).tiny
        assert (d["subnormal"] > 0).all() and (d["subnormal"] < tiny).all()
        assert np.abs(d["large"]).max() > 1e149 and np.isfinite(np.square(d["large"]).sum())
        assert np.isinf(d["inf1"]).sum() == 1
        if n >= 2:
            assert (d["inf2"] == np.inf).sum() == 1 and (d["inf2"] == -np.inf).sum() == 1
        for r in EL.nan_rows(n):
            x = d["nan@%d" % r]
            assert np.isnan(x[r]) and np.isnan(x).sum() == 1
        for k in ("f32w", "f32w.pos"):
            assert (d[k].view(np.uint64) & np.uint64((1 << 29) - 1) == 0).all()
        assert EL.is_normal_finite(d["randn"]) and not EL.is_normal_finite(d["subnormal"]) and not EL.is_normal_finite(d["inf1"])


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("family", FAMILIES)
def test_percentile_methods_differ(family, n):
    x = EL.sharp_columns(n)[family]
    for q in (10, 90):
        g = _gamma_tenths(n, float(q))
        lin = np.percentile(x, q)
        for method in ("lower", "higher", "midpoint"):
            same = g == 0.0 or (method == "midpoint" and g == 0.5)
            assert (np.percentile(x, q, method=method) == lin) == same, (family, n, q, method)
        # one half of _lerp used for every gamma: the other form rounds differently somewhere, but not at every n; counted below
    if n % 2 == 0:
        assert np.sort(x)[n // 2] != np.median(x), (family, n)           # the upper middle element taken for the median
    else:
        s = np.sort(x)
        assert s[n // 2 - 1] != np.median(x), (family, n)                # x[3] for x[4] in the kernel's odd case


def test_lerp_halves_differ_somewhere():
    """`b - diff * (1 - t)` used for every t differs from NumPy's two-sided _lerp on several committed columns with t < 0.5 (the two forms
    round alike more often than not, so this is counted over every finite column rather than asserted per column)."""
    hits = 0
    for n in NS:
        for name, x in EL.summary_columns(n):
            if not EL.is_normal_finite(x):
                continue
            s = np.sort(x)
            for q in (10.0, 90.0):
                v = (n - 1) * (q / 100.0)
                g = v - math.floor(v)
                if 0 < g < 0.5:
                    a, b = s[int(v)], s[int(v) + 1]
                    hits += (b - (b - a) * (1 - g)) != np.percentile(x, q)
    print("columns where the one-sided lerp differs:", hits)
    assert hits >= 5, hits


@pytest.mark.parametrize("n", NS)
def test_lowest_key_byte_decides(n):
    """A selection that ignores the lowest key byte returns other order statistics on family 2."""
    for name in ("lowbyte", "lowbyte.neg"):
        x = dict(EL.summary_columns(n))[name]
        k = EL.key_of(x) & ~np.uint64(255)
        b = np.where(k >> np.uint64(63), k & np.uint64((1 << 63) - 1), ~k)              # value_of
        wrong = EL.stats_by_order(b.view(np.float64), np.argsort(k, kind="stable"))
        true = EL.stats_by_order(x, np.argsort(x, kind="stable"))
        assert true == [EL.stats_of(x)[s] for s in EL.ORDER_STATS]
        assert sum(w != t for w, t in zip(wrong, true)) >= 3, (n, name, wrong, true)


@pytest.mark.parametrize("n", NS)
def test_raw_bit_order_misorders_mixed_signs(n):
    """Comparing the raw bit patterns as signed integers (no key_of flip) reverses the negatives of family 1."""
    x = dict(EL.summary_columns(n))["randn"]
    true = EL.stats_by_order(x, np.argsort(x, kind="stable"))
    assert true == [EL.stats_of(x)[s] for s in EL.ORDER_STATS]
    assert (np.argsort(EL.key_of(x), kind="stable") == np.argsort(x, kind="stable")).all()       # the kernel's key orders as the values do
    if (x < 0).sum() >= 2:
        wrong = EL.stats_by_order(x, np.argsort(x.view(np.int64), kind="stable"))
        assert wrong != true, (n, wrong, true)
    else:
        assert n < 8


@pytest.mark.parametrize("A", EL.METRIC_AGENTS)
def test_sum_order_over_agents_shows(A):
    """Sequential summation over agents differs bitwise from np.sum in at least 10 % of the rows for A >= 8 on every summed input; the
    transcription of the kernel's np_sum equals np.sum / np.mean on all of them for every A."""
    fi, ret, _ = EL.metrics_inputs(1000, A)
    f64 = fi.astype(np.float64)
    cols = [("ret", ret)] + [(key, f64[..., EL.K[key]]) for _, key, _ in EL.SUMMED]
    for name, x in cols:
        rows = [r.tolist() for r in x]
        ref = [np.sum(r) for r in rows]
        assert [EL.kernel_np_sum(r) for r in rows] == ref, (A, name)
        assert [EL.kernel_np_sum(r) / A for r in rows] == [np.mean(r) for r in rows], (A, name)
        differ = sum(EL.sequential_sum(r) != s for r, s in zip(rows, ref))
        print("A=%d %s: sequential != np.sum in %d of %d rows" % (A, name, differ, len(rows)))
        if A >= 8:
            assert differ >= 0.10 * len(rows), (A, name, differ)
    # the rows of every Time_req_to_goal pattern exist at N = 1000, and N = 1 meets each pattern at some A
    pats = {EL.row_pattern(i, A) for i in range(1000)}
    assert pats == set(EL.ROW_PATTERNS)


def test_metrics_inputs_cover_the_edges():
    assert {EL.row_pattern(0, A) for A in EL.METRIC_AGENTS} >= {"all -1", "none -1", "nan first", "nan middle", "nan last", "mix"}
    for N in EL.METRIC_ENVS:
        for A in (1, 16, 64):
            fi, ret, steps = EL.metrics_inputs(N, A)
            t = fi[..., EL.K["Time_req_to_goal"]]
            for i in range(N):
                p = EL.row_pattern(i, A)
                assert np.isnan(t[i]).sum() == p.startswith("nan")
                if p == "all -1":
                    assert (t[i] == -1).all()
                if p == "none -1":
                    assert (t[i] != -1).all()
            assert (fi[..., EL.K["Dist_to_goal"]] == np.float32(EL.METRIC_THRESH)).any()
            if N >= 4:
                assert (fi[1::4, A - 1, EL.K["Distance_variance"]] == np.float32(-0.0001)).all()
                big = 1.0 / (fi[1, A - 1, EL.K["Distance_variance"]].astype(np.float64) + 0.0001)
                assert abs(big) > 1e10


def test_exact_references_and_bounds():
    rng = np.random.RandomState(3)
    for n in (1, 2, 17, 1000):
        x = rng.randn(n) * 10.0 ** rng.randint(-5, 6, n)
        m, var, sabs = EL.exact_moments(x)
        assert float(m) == math.fsum(x) / n or abs(float(m) - math.fsum(x) / n) <= 2.0 ** -52 * abs(float(m))
        np.testing.assert_allclose([float(m), math.sqrt(float(var)), float(sabs)], [np.mean(x), np.std(x), np.abs(x).sum()], rtol=1e-10)
        EL.check_mean_std(x, float(np.mean(x)), float(np.std(x)))                  # NumPy's own two-pass result is inside the derived bounds
        if n > 2:
            with pytest.raises(AssertionError):
                EL.check_mean_std(x, float(np.mean(x)) + 1e-9 * np.abs(x).sum(), float(np.std(x)))
            with pytest.raises(AssertionError):
                EL.check_mean_std(x, float(np.mean(x)), float(np.std(x)) * (1 + 1e-9))
    EL.check_mean_std(np.full(7, 0.1), float(np.mean(np.full(7, 0.1))), float(np.std(np.full(7, 0.1))))
    with pytest.raises(AssertionError):
        EL.check_sums([1.0 + 1e-9], [[0.25, 0.75]])
    with pytest.raises(AssertionError):
        EL.check_sums([1.0, 1.0], [[0.25, 0.75], [1.0, float("nan")]])
    EL.check_sums([1.0, float("nan")], [[0.25, 0.75], [1.0, float("nan")]])
    x = rng.randn(50, 33) * 10.0 ** rng.randint(-8, 9, (50, 33))
    EL.check_sums(x.sum(1), x)
    EL.check_sums([EL.sequential_sum(r) / 33 for r in x.tolist()], x, 33)
    # a one-pass variance (E x^2 - m^2) fails the bound where the offset dwarfs the spread: the two-pass claim is checked, not assumed
    x = 1e6 + rng.randn(1000)
    with pytest.raises(AssertionError):
        EL.check_mean_std(x, float(np.mean(x)), math.sqrt(abs(np.mean(x * x) - np.mean(x) ** 2)))
    # the 1e-12 agreement with NumPy applies to the one-signed columns at every row count
    assert all(EL.numpy_agreement(dict(EL.summary_columns(n))["f32w.pos"])[0] for n in EL.SUMMARY_NS)
    assert EL.numpy_agreement(dict(EL.summary_columns(100003))["f32w.pos"]) == (True, True)


def test_record_cases_cover_every_shape_and_width():
    cases = EL.record_cases()
    assert {(c[0], c[1]) for c in cases} == set(EL.RECORD_SHAPES)
    assert {c[2] for c in cases} == set(EL.RECORD_ACTIONS) and {c[3] for c in cases} == set(EL.RECORD_RNN_ROWS)
    assert {c[4] for c in cases} == set(EL.RECORD_STEPS)
    for N, A in EL.RECORD_SHAPES:
        mine = [c for c in cases if (c[0], c[1]) == (N, A)]
        assert {c[3] for c in mine} == set(EL.RECORD_RNN_ROWS), (N, A)
        assert {c[2] for c in mine} >= {1, 2, 24, 25} and {c[4] for c in mine} == {1, 2, 25}
    assert all(c[0] <= 33 for c in cases if c[2] == 4096) and len(cases) == len(set(cases))
    rng = np.random.RandomState(0)
    for A, T in ((1, 1), (5, 25), (64, 25), (64, 2)):
        never, one, seq, froz, last = [EL.done_schedule(rng, p, A, T) for p in EL.DONE_PATTERNS]
        assert not never.any() and one.all(1).sum() == 1 and froz[0].all() and not last.all(1).any()
        assert (np.diff(seq.sum(1)) >= 0).all() and seq[-1].all() == (T > 1 or True)
        if T == 25:
            assert (np.diff(seq.sum(1)) > 0).any() and last.any()
    rew, done, info = EL.record_inputs(33, 5, 25, 1)
    iv = info.view(np.int32)
    assert np.isnan(info).any() and (iv == -2 ** 31).any() and len(set(iv[np.isnan(info)].tolist())) == 2
