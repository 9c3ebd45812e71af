"""GPU parity of the period kernels (``k_row_period``, ``k_tail_score`` on the period planes) and of the period step of a
report against the NumPy restatement of tests/period_oracle_backend.py.  Every row of every case is compared.

Bounds (include/nvrx_straggler.h has the definition), by the onset test's own argument.  The kernel and NumPy add the same f64
numbers in different orders: f64 roundoff is 1.1e-16, times 65 536 additions that is 7e-12 relative on a phase sum, and
B_P / SST squares such sums; the adjustment (n - 1) / (n - P) <= 4 / 3 amplifies the result no further -- 1e-9 absolute on a
strength of at most 1 leaves about 100 x.  The record carries the strength as f32, so the record's value is compared with the
oracle's f64 a at the kernel's P* within 1e-9 plus half an f32 ulp at that value.  ``peak`` / ``rest``: within one f32 ulp
where the period and the slow phase agree with the oracle's.  The choice: the oracle's a at the kernel's period is
>= 0.95 * a_max - 1e-9, and no smaller period has an oracle a >= 0.95 * a_max + 1e-9; a row of which no candidate lies inside
that 1e-9 band must show the oracle's very period, and no more than 2 % of a case's rows may lie inside it
(tests/test_period_host.py checks that on the oracle alone).  On every planted row the period is the planted one and ``ago`` the
oracle's.  Absent, short, constant and non-finite rows are compared exactly.

Five consecutive slow samples in every two are a constant row: period 2 is planted with one slow sample only."""
import numpy as np
import pytest
import torch

import period_workers
from period_oracle_backend import choose, period_excess, period_scores_table, phase_means, row_period, row_period_one
from test_gpu_score import _random_table

pytestmark = pytest.mark.gpu

TOL = 1e-9
_worst = {"strength": 0.0, "below_bar": 0.0, "ulp": 0.0, "band_rows": 0}


@pytest.fixture(scope="module")
def be():
    from nvrx_straggler.backend import get_backend

    return get_backend()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _period(be, samples, counts, max_period, starts=None):
    s = torch.from_numpy(np.ascontiguousarray(samples, dtype=np.float32)).cuda()
    c = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int32)).cuda()
    st = None if starts is None else torch.from_numpy(np.ascontiguousarray(starts, dtype=np.int32)).cuda()
    raw = be.row_period(s, c, max_period, st).cpu().numpy()
    rec = np.ascontiguousarray(raw).view(np.uint32)
    return (rec[:, 0] & 0xFFFF, rec[:, 0] >> 16, rec[:, 1].copy().view(np.float32), rec[:, 2].copy().view(np.float32),
            rec[:, 3].copy().view(np.float32))


def _within_one_ulp(got, want):
    d = abs(float(got) - float(want)) / float(np.spacing(np.abs(np.float32(want))))
    _worst["ulp"] = max(_worst["ulp"], d)
    return d <= 1.0


def _check(be, samples, counts, max_period, planted, tag, starts=None):
    period, ago, peak, rest, strength = _period(be, samples, counts, max_period, starts)
    exp, curves, phases, ordered = row_period(samples, counts, max_period, starts)
    band = set(period_workers.band_rows(curves))
    _worst["band_rows"] = max(_worst["band_rows"], len(band))
    assert len(band) <= 0.02 * samples.shape[0], (tag, sorted(band))
    for r in range(samples.shape[0]):
        n = min(int(counts[r]), samples.shape[1])
        got = (int(period[r]), int(ago[r]), peak[r], rest[r], strength[r])
        e = exp[r]
        where = (tag, r, n, got, e)
        curve = curves[r]
        if curve is None:
            # absent, non-finite, short or constant: exact (NaN by NaN-ness)
            assert got[0] == 0 and got[1] == 0, where
            if np.isnan(e["strength"]):
                assert np.isnan(got[2]) and np.isnan(got[3]) and np.isnan(got[4]), where
            else:
                assert _bits(got[4]) == _bits(e["strength"]), where
                assert _within_one_ulp(got[2], e["peak"]) and _within_one_ulp(got[3], e["rest"]) and _bits(got[2]) == _bits(got[3]), where
                if n == 0 or ordered[r] is None or np.all(ordered[r] == ordered[r][0]):  # (absent / constant: bit-exact)
                    assert _bits(got[2]) == _bits(e["peak"]), where
            continue
        a_max = float(curve.max())
        P = got[0]
        if P == 0:  # the kernel found no period: nothing explains anything
            assert a_max <= TOL and got[1] == 0 and got[4] == 0.0, where + (a_max,)
            assert _within_one_ulp(got[2], e["peak"] if e["period"] == 0 else got[2]) and _bits(got[2]) == _bits(got[3]), where
        else:
            assert 2 <= P <= min(max_period, n // 4) and got[1] < P, where
            at = float(curve[P - 2])
            _worst["below_bar"] = max(_worst["below_bar"], 0.95 * a_max - at)
            assert a_max > -TOL and at >= 0.95 * a_max - TOL, where + (a_max, at)
            assert not np.any(curve[: P - 2] >= 0.95 * a_max + TOL), where + (a_max,)
            d = abs(float(got[4]) - at)
            _worst["strength"] = max(_worst["strength"], max(0.0, d - 0.5 * float(np.spacing(np.float32(at)))))
            assert d <= TOL + 0.5 * float(np.spacing(np.float32(at))), where + (d,)
            S, cnt = phase_means(ordered[r], P)
            f = (n - 1 - got[1]) % P  # the kernel's slow phase: its mean is the oracle's largest (to the bound's precision)
            means = S / cnt
            assert means[f] >= means.max() - 1e-9 * max(1.0, abs(means.max())), where + (f,)
        if r not in band:
            assert P == int(e["period"]), where
        if planted[r]:
            assert P == planted[r] and P == int(e["period"]) and got[1] == int(e["ago"]), where + (planted[r],)
        if P and P == int(e["period"]) and (n - 1 - got[1]) % P == phases[r]:
            assert _within_one_ulp(got[2], e["peak"]) and _within_one_ulp(got[3], e["rest"]), where


@pytest.mark.parametrize("stride", period_workers.STRIDES)
def test_row_period_every_stride_count_and_data_kind(be, stride):
    """Every data kind at every count, every planted period that fits: strides 8 .. 65 536, one either side of the LDS
    boundary (rows of up to 10 240 samples are staged)."""
    samples, counts, max_period, planted = period_workers.kernel_case(stride)
    assert planted.any()
    _check(be, samples, counts, max_period, planted, ("stride", stride))
    print(f"stride {stride}: {samples.shape[0]} rows, worst so far {_worst}")


@pytest.mark.parametrize("stride", [64, 1000, 4100, period_workers.LDS_SAMPLES + 4])
def test_row_period_ring_starts(be, stride):
    """Full rows whose oldest sample lives in slot 0, 1, 3, n/2 and n-1: the rotated rows give the records of the unrotated
    ones, bit for bit.  The planted periods do not divide the rows' length."""
    samples, counts, starts, max_period, planted = period_workers.rotation_case(stride)
    assert planted.any() and all(stride % P for P in planted if P)
    _check(be, samples, counts, max_period, planted, ("starts", stride), starts=starts)
    got = _period(be, samples, counts, max_period, starts)
    for base in range(0, samples.shape[0], 5):  # the same samples in time order: the very same arithmetic
        for q in got:
            assert all(_bits(q[base + j]) == _bits(q[base]) for j in range(1, 5)), (stride, base)
    again = _period(be, samples, counts, max_period, starts)  # ... and from launch to launch
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, again))


@pytest.mark.parametrize("rows,stride", [(1, 10000), (512, 1000), (4096, 256)])
def test_row_period_launch_sizes(be, rows, stride):
    samples, counts, max_period, planted = period_workers.launch_case(rows, stride)
    _check(be, samples, counts, max_period, planted, ("launch", rows, stride))
    print(f"launch {rows} x {stride}: worst so far {_worst}")


# ---- nvrx_period_score ------------------------------------------------------------------------------------------------------
def _random_periods(rng, R, K, S, p_missing=0.15):
    KS = K + S
    o = np.full((R, 7, KS), -1.0, dtype=np.float32)
    have = rng.random((R, KS)) >= p_missing
    excess = np.where(rng.random((R, KS)) < 0.5, 1.0, rng.uniform(1.0, 3.0, (R, KS))).astype(np.float32)
    o[:, 0, :] = np.where(have, excess, -1.0)
    for p in range(1, 7):  # (the other planes are not read: anything but the excesses)
        o[:, p, :] = np.where(have, rng.uniform(0.0, 100.0, (R, KS)), -1.0)
    return o


def _period_score(be, periods, T, K, S, first_rank=0, n_ranks=None):
    R = T.shape[0]
    ws = be.workspace(R, K, S, R, 0)
    ws.period_settle()
    ws.send.copy_(torch.from_numpy(T))
    _, table, _, _ = ws.period_buffers()
    if table.numel():
        table.copy_(torch.from_numpy(periods.reshape(R, -1)))
    torch.cuda.synchronize()
    handle = be.period_score(ws, table, ws.send, first_rank, n_ranks)
    got_periods, scores = handle.records()
    lo = first_rank
    hi = R if n_ranks is None else first_rank + n_ranks
    assert np.array_equal(_bits(got_periods), _bits(periods[lo:hi]))  # the planes are returned unchanged
    return scores


@pytest.mark.parametrize("R,K,S", [(1, 3, 0), (8, 5, 6), (64, 17, 33), (65, 0, 64), (100, 7, 9)])
def test_period_score_matches_numpy(be, R, K, S):
    rng = np.random.default_rng(R * 1000 + K + S)
    T = _random_table(rng, R, K, S)
    periods = _random_periods(rng, R, K, S)
    if R > 1 and K + S > 2:
        periods[:, 0, 1] = rng.uniform(1.0, 2.0, R)  # a column nobody misses
    got = _period_score(be, periods, T, K, S)
    exp = period_scores_table(periods, T, K, S)
    assert got.shape == exp.shape == (R, 1 + S)
    assert np.array_equal(np.isnan(got), np.isnan(exp))
    sec_ok = ~np.isnan(exp[:, 1:])
    assert np.array_equal(_bits(got[:, 1:][sec_ok]), _bits(exp[:, 1:][sec_ok]))  # one f64 quotient rounded to f32
    gpu_ok = np.isfinite(exp[:, 0])
    if gpu_ok.any():
        assert np.abs(got[gpu_ok, 0].astype(np.float64) - exp[gpu_ok, 0].astype(np.float64)).max() <= 2e-6
    lo, n = (R // 3, max(1, R // 2)) if R > 1 else (0, 1)
    part = _period_score(be, periods, T, K, S, lo, n)
    assert np.array_equal(_bits(part), _bits(got[lo : lo + n]))


def test_period_local_needs_the_ring_start_snapshot(be):
    """Without ``nvrx_onset_enable`` no report has noted where the rings start: NVRX_ERR_STATE (-1), nothing launched."""
    from nvrx_straggler import _native

    rings = be.make_rings(1, 4, 64)
    buf = torch.empty(7 * 4, dtype=torch.float32, device="cuda")
    try:
        rc = be.lib.nvrx_period_local(rings.ctx, None, 1024, 0.5, buf.data_ptr(), 0, 4, 0, be.stream_handle)
        assert rc == -1 and b"snapshot" in be.lib.nvrx_last_error()
    finally:
        rings.close()


# ---- the period step of a report ----------------------------------------------------------------------------------------------
from mp_util import run_ranks  # noqa: E402
from test_period_host import check_headline  # noqa: E402


def _check_record(rec, x, max_period, where):
    """One record of a report against the oracle on the row ``x`` (time order): the period and the slow phase are the
    oracle's, the rest within the bounds above."""
    (period, ago, peak, rest, strength), curve, _ = row_period_one(x, max_period)
    assert rec["period"] == int(period) and rec["samples_ago"] == int(ago) and rec["window"] == x.size, (where, rec, period, ago)
    assert abs(rec["strength"] - float(strength)) <= 1.2e-7, (where, rec, strength)  # (one f32 ulp below 1)
    assert abs(rec["peak"] - float(peak)) <= float(np.spacing(peak)), (where, rec, peak)
    assert abs(rec["rest"] - float(rest)) <= float(np.spacing(rest)), (where, rec, rest)
    assert rec["excess"] == float(period_excess(rec["period"], rec["peak"], rec["rest"], rec["strength"], 0.5)), (where, rec)


def _check_headline_gpu(s, data):
    """The headline's bounds, and every record against the oracle."""
    check_headline(s, data, exact=False)
    for i, (name, per) in enumerate(sorted(s["periods"]["section_periods"].items())):
        for r, rec in per.items():
            if r == period_workers.BEAT_RANK:
                _check_record(rec, data[r, i], 1024, (name, r))
            else:  # (noise: which of many weak periods wins is the row-kernel tests' matter)
                curve = row_period_one(data[r, i], 1024)[1]
                assert abs(rec["strength"] - float(curve[rec["period"] - 2])) <= 1e-9 + 6e-8 if rec["period"] else rec["strength"] == 0.0
                assert rec["excess"] == 1.0


def test_headline_shape_in_one_process(be):
    data = period_workers.headline_data()
    out = period_workers.folded_headline(0, 1)
    assert len(out) == 3
    for entry in out:
        _check_headline_gpu(entry["report"], data)
        assert entry["report"]["tails"] == {} and entry["report"]["onsets"] == {}
        assert entry["rows"] == []  # (one process: nothing is exchanged)


@pytest.mark.parametrize("world,tail_quantile,onset_detection", [(2, 0.0, False), (4, 0.95, True)])
def test_headline_shape_on_processes_sharing_the_gpu(world, tail_quantile, onset_detection):
    """Default route (gloo / c10d); with four processes tail and onset scores are on as well: three follow-up steps behind one
    report, each with its own all-gather."""
    data = period_workers.headline_data()
    res = run_ranks(period_workers.folded_headline, world, timeout=300, use_oracle_backend=False, device=0,
                    tail_quantile=tail_quantile, onset_detection=onset_detection)
    follow_ups = 1 + bool(tail_quantile) + bool(onset_detection)
    for r in range(world):
        assert all((e["report"] is None) == (r != 0) for e in res[r])
        for i, e in enumerate(res[r]):
            # every rank: the report's own all-gather (the first report exchanges twice: once before the name sync that
            # gives its names their ids, once after), then exactly one per follow-up step, the period rows last
            assert len(e["rows"]) == (2 if i == 0 else 1) + follow_ups and e["rows"][-1] % 7 == 0, (r, i, e["rows"])
            KS = e["rows"][-1] // 7
            if follow_ups == 3:
                assert e["rows"][-3:] == [KS, 6 * KS, 7 * KS], (r, e["rows"])
    for e in res[0]:
        rep = e["report"]
        _check_headline_gpu(rep, data)
        assert bool(rep["tails"]) == bool(tail_quantile) and bool(rep["onsets"]) == bool(onset_detection)
        if tail_quantile:
            assert rep["tails"]["quantile"] == tail_quantile and sorted(rep["tails"]["section_tails"]) == sorted(
                rep["periods"]["section_periods"]) == sorted(rep["onsets"]["section_onsets"])


@pytest.mark.parametrize("asynchronous", [False, True])
def test_next_window_written_from_another_stream_right_after_the_report(asynchronous):
    """The ordering rule: the period kernel has read its window before the report call returns."""
    res = run_ranks(period_workers.ring_windows_written_from_another_stream, 1, timeout=300, use_oracle_backend=False, device=0,
                    asynchronous=asynchronous)[0]
    samples, names, beats = res["samples"], res["names"], res["beats"]
    assert len(res["reports"]) == samples.shape[0] == 12
    for w, rep in enumerate(res["reports"]):
        for s, name in enumerate(names):
            rec = rep["section_periods"][name]
            _check_record(rec, samples[w, s], 128, (w, name))
            assert rec["period"] == int(beats[w, s]) and abs(rec["excess"] - 1.5) < 0.02, (w, name, rec, beats[w, s])
        # every section stalls by the same factor: one rank is its own reference
        assert all(v == 1.0 for v in rep["section_relative"].values())
        at_return, before_read, after_first, after_second = rep["copy_outs"]
        # neither the report call nor scores / stragglers copy periods out; the first period_scores() does, exactly once
        assert at_return == before_read == w and after_first == after_second == w + 1, (w, rep["copy_outs"])


def test_wrapped_ring_is_walked_in_time_order():
    """1.5 x ring_cap samples (and 2 x + 5) pushed into 64-deep rings, between windows that do not wrap."""
    res = run_ranks(period_workers.wrapped_ring, 1, timeout=300, use_oracle_backend=False, device=0)[0]
    assert len(res["windows"]) == 4
    for w in res["windows"]:
        pushed = w["pushed"]
        n = min(pushed.shape[1], 64)
        for s, name in enumerate(res["names"]):
            rec = w["periods"][name][0]
            _check_record(rec, pushed[s, -n:], 1024, name)
            assert rec["period"] == 4 + s and abs(rec["excess"] - 1.5) < 0.03, (name, rec)
