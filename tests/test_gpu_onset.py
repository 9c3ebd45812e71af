"""GPU parity of the onset kernels (``k_row_onset``, ``k_tail_score`` on the onset planes) and of the onset step of a report
against the NumPy restatement of tests/onset_oracle_backend.py.  Every row of every case is compared.

Bounds (include/nvrx_straggler.h has the definition).  The kernel and NumPy add the same f64 numbers in different orders:
f64 roundoff is 1.1e-16, times 65 536 additions that is 7e-12 relative on a prefix sum, and D / SST squares a difference of
two of them -- 1e-9 absolute on a strength in [0, 1] leaves about 100 x.  The record carries the strength as f32, so the
record's value is compared with the oracle's f64 strength within 1e-9 plus half an f32 ulp at that value (the rounding of
the format, 3e-8 near 1).  ``before`` / ``after``: within one f32 ulp.  The split: the oracle's strength at the kernel's t* is
within 1e-9 of the oracle's maximum, and wherever the oracle's runner-up is further below the maximum than that, t* is equal.
Constant rows, short rows, absent rows and non-finite rows are compared exactly."""
import numpy as np
import pytest
import torch

from onset_oracle_backend import min_segment, onset_scores_table, row_onset
from test_gpu_score import _random_table

pytestmark = pytest.mark.gpu

SEG_PPM = 50000
TOL = 1e-9
KINDS = ("noise", "step_5", "step_50", "step_95", "step_down", "ramp", "constant", "two_steps", "one_nan", "one_inf")
_worst = {"strength": 0.0, "at_split": 0.0, "ulp": 0.0}


@pytest.fixture(scope="module")
def be():
    from nvrx_straggler.backend import get_backend

    return get_backend()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _row(kind, rng, n):
    """One row of ``n`` samples around 1000 with 1 % noise."""
    x = 1000.0 * (1.0 + 0.01 * rng.standard_normal(n))
    if kind.startswith("step_") and kind != "step_down":
        x[int(n * int(kind[5:]) / 100):] *= 1.5
    elif kind == "step_down":
        x[n // 3:] *= 0.6
    elif kind == "ramp":
        x += np.arange(n) * (300.0 / max(n, 1))
    elif kind == "constant":
        x[:] = 1234.5
    elif kind == "two_steps":
        x[n // 4:] *= 1.2
        x[(2 * n) // 3:] *= 1.4
    elif kind == "one_nan":
        x[n // 2] = np.nan
    elif kind == "one_inf":
        x[n // 3] = np.inf
    return x.astype(np.float32)


def _onset(be, samples, counts, starts=None, seg_ppm=SEG_PPM):
    s = torch.from_numpy(np.ascontiguousarray(samples, dtype=np.float32)).cuda()
    c = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int32)).cuda()
    st = None if starts is None else torch.from_numpy(np.ascontiguousarray(starts, dtype=np.int32)).cuda()
    raw = be.row_onset(s, c, seg_ppm, st).cpu().numpy()
    rec = np.ascontiguousarray(raw).view(np.uint32)
    return rec[:, 0].copy(), rec[:, 1].copy().view(np.float32), rec[:, 2].copy().view(np.float32), rec[:, 3].copy().view(np.float32)


def _within_one_ulp(got, want):
    d = abs(float(got) - float(want)) / float(np.spacing(np.abs(np.float32(want))))
    _worst["ulp"] = max(_worst["ulp"], d)
    return d <= 1.0


def _check(be, samples, counts, tag, starts=None, expect_equal_split=()):
    ago, before, after, strength = _onset(be, samples, counts, starts)
    exp, curves = row_onset(samples, counts, SEG_PPM, starts)
    for r in range(samples.shape[0]):
        n = min(int(counts[r]), samples.shape[1])
        got = (int(ago[r]), before[r], after[r], strength[r])
        e = exp[r]
        where = (tag, r, n, got, e)
        if curves[r] is None:
            # absent, non-finite, short or constant: exact (NaN by NaN-ness)
            assert got[0] == int(e["ago"]), where
            if np.isnan(e["strength"]):
                assert np.isnan(got[1]) and np.isnan(got[2]) and np.isnan(got[3]), where
            else:
                assert _bits(got[3]) == _bits(e["strength"]), where
                assert _within_one_ulp(got[1], e["before"]) and _within_one_ulp(got[2], e["after"]), where
                if n == 0 or (n >= 2 * min_segment(SEG_PPM, n)):  # (absent / constant: bit-exact)
                    assert _bits(got[1]) == _bits(e["before"]) and _bits(got[2]) == _bits(e["after"]), where
            continue
        curve = curves[r]  # the oracle's f64 strength at every admissible split t = m .. n - m
        m = min_segment(SEG_PPM, n)
        best = int(np.argmax(curve))
        top = float(curve[best])
        t_got = n - got[0]
        assert m <= t_got <= n - m, where
        at_split = top - float(curve[t_got - m])
        _worst["at_split"] = max(_worst["at_split"], at_split)
        assert at_split <= TOL, where + (at_split,)
        runner_up = float(np.max(np.delete(curve, best))) if curve.size > 1 else -np.inf
        if top - runner_up > TOL or r in expect_equal_split:
            assert t_got == best + m, where + (top - runner_up,)
        d = abs(float(got[3]) - top)
        _worst["strength"] = max(_worst["strength"], max(0.0, d - 0.5 * float(np.spacing(np.float32(top)))))
        assert d <= TOL + 0.5 * float(np.spacing(np.float32(top))), where + (d,)
        if t_got == best + m:
            assert _within_one_ulp(got[1], e["before"]) and _within_one_ulp(got[2], e["after"]), where


def _counts_for(stride):
    return [min(c, stride) for c in (0, 1, 15, 16, 17, 33, stride)]


@pytest.mark.parametrize("stride", [4, 8, 64, 256, 1000, 1024, 4096, 4100, 5000, 10000, 65536])
def test_row_onset_every_stride_count_and_data_kind(be, stride):
    """Every data kind at every count: 70 rows per launch.  On the stepped full rows the split must be the oracle's."""
    rng = np.random.default_rng(stride)
    counts, rows, stepped = [], [], []
    for kind in KINDS:
        for c in _counts_for(stride):
            row = np.zeros(stride, dtype=np.float32)
            row[:] = _row(kind, rng, stride)
            if kind.startswith("step") and c == stride and stride >= 64:
                stepped.append(len(rows))
            rows.append(row)
            counts.append(c)
    _check(be, np.stack(rows), np.array(counts, dtype=np.uint32), ("stride", stride), expect_equal_split=set(stepped))
    print(f"stride {stride}: worst so far {_worst}")


@pytest.mark.parametrize("stride", [64, 1000, 4100, 65536])
def test_row_onset_ring_starts(be, stride):
    """Full rows whose oldest sample lives in slot 0, 1, 3, n/2 and n-1: the rotated rows give the records of the unrotated ones."""
    rng = np.random.default_rng(stride + 1)
    rows, starts, stepped = [], [], []
    for kind in KINDS:
        x = _row(kind, rng, stride)
        for start in (0, 1, 3, stride // 2, stride - 1):
            if kind.startswith("step"):
                stepped.append(len(rows))
            rows.append(np.roll(x, start))
            starts.append(start)
    samples, counts = np.stack(rows), np.full(len(rows), stride, dtype=np.uint32)
    _check(be, samples, counts, ("starts", stride), starts=np.array(starts, dtype=np.uint32), expect_equal_split=set(stepped))
    got = _onset(be, samples, counts, np.array(starts, dtype=np.uint32))
    for base in range(0, len(rows), 5):  # the same samples in time order: the very same arithmetic
        for q in got:
            assert all(_bits(q[base + j]) == _bits(q[base]) or (np.isnan(q[base + j]) and np.isnan(q[base])) for j in range(1, 5))


@pytest.mark.parametrize("rows,stride", [(1, 10000), (512, 10000), (4096, 1000)])
def test_row_onset_launch_sizes(be, rows, stride):
    rng = np.random.default_rng(rows)
    samples = np.stack([_row(KINDS[r % len(KINDS)], rng, stride) for r in range(rows)])
    counts = np.full(rows, stride, dtype=np.uint32)
    counts[5::11] = rng.integers(0, stride + 1, counts[5::11].size)
    stepped = {r for r in range(rows) if KINDS[r % len(KINDS)].startswith("step") and counts[r] == stride}
    _check(be, samples, counts, ("launch", rows, stride), expect_equal_split=stepped)
    print(f"launch {rows} x {stride}: worst so far {_worst}")


# ---- nvrx_onset_score -------------------------------------------------------------------------------------------------------
def _random_onsets(rng, R, K, S, p_missing=0.15):
    KS = K + S
    o = np.full((R, 6, KS), -1.0, dtype=np.float32)
    have = rng.random((R, KS)) >= p_missing
    shift = np.where(rng.random((R, KS)) < 0.5, 1.0, rng.uniform(1.0, 3.0, (R, KS))).astype(np.float32)
    o[:, 0, :] = np.where(have, shift, -1.0)
    for p in range(1, 6):  # (the other planes are not read: anything but the shifts)
        o[:, p, :] = np.where(have, rng.uniform(0.0, 100.0, (R, KS)), -1.0)
    return o


def _onset_score(be, onsets, T, K, S, first_rank=0, n_ranks=None):
    R = T.shape[0]
    ws = be.workspace(R, K, S, R, 0)
    ws.onset_settle()
    ws.send.copy_(torch.from_numpy(T))
    _, table, _, _ = ws.onset_buffers()
    if table.numel():
        table.copy_(torch.from_numpy(onsets.reshape(R, -1)))
    torch.cuda.synchronize()
    handle = be.onset_score(ws, table, ws.send, first_rank, n_ranks)
    got_onsets, scores = handle.records()
    lo = first_rank
    hi = R if n_ranks is None else first_rank + n_ranks
    assert np.array_equal(_bits(got_onsets), _bits(onsets[lo:hi]))
    return scores


@pytest.mark.parametrize("R,K,S", [(1, 3, 0), (8, 5, 6), (64, 17, 33), (65, 0, 64), (100, 7, 9)])
def test_onset_score_matches_numpy(be, R, K, S):
    rng = np.random.default_rng(R * 1000 + K + S)
    T = _random_table(rng, R, K, S)
    onsets = _random_onsets(rng, R, K, S)
    if R > 1 and K + S > 2:
        onsets[:, 0, 1] = rng.uniform(1.0, 2.0, R)  # a column nobody misses
    got = _onset_score(be, onsets, T, K, S)
    exp = onset_scores_table(onsets, T, K, S)
    assert got.shape == exp.shape == (R, 1 + S)
    assert np.array_equal(np.isnan(got), np.isnan(exp))
    sec_ok = ~np.isnan(exp[:, 1:])
    assert np.array_equal(_bits(got[:, 1:][sec_ok]), _bits(exp[:, 1:][sec_ok]))  # one f64 quotient rounded to f32
    gpu_ok = np.isfinite(exp[:, 0])
    if gpu_ok.any():
        assert np.abs(got[gpu_ok, 0].astype(np.float64) - exp[gpu_ok, 0].astype(np.float64)).max() <= 2e-6
    lo, n = (R // 3, max(1, R // 2)) if R > 1 else (0, 1)
    part = _onset_score(be, onsets, T, K, S, lo, n)
    assert np.array_equal(_bits(part), _bits(got[lo : lo + n]))


# ---- the onset step of a report -----------------------------------------------------------------------------------------------
import onset_workers  # noqa: E402
from mp_util import run_ranks  # noqa: E402
from onset_oracle_backend import onset_shift, row_onset_one  # noqa: E402
from test_onset_host import check_headline  # noqa: E402


def _check_headline_gpu(s, data):
    """The headline's bounds, and every record against the oracle."""
    check_headline(s, data, exact=False)
    for i, (name, per) in enumerate(sorted(s["onsets"]["section_onsets"].items())):
        for r, rec in per.items():
            (ago, before, after, strength), _ = row_onset_one(data[r, i], SEG_PPM)
            assert abs(rec["strength"] - float(strength)) <= 1.2e-7, (name, r, rec, strength)  # (one f32 ulp below 1)
            assert abs(rec["before"] - float(before)) <= float(np.spacing(before)), (name, r)
            assert abs(rec["after"] - float(after)) <= float(np.spacing(after)), (name, r)
            if r == onset_workers.STEP_RANK:
                assert rec["samples_ago"] == int(ago) == 600, (name, rec)
                assert rec["shift"] == float(np.float32(np.float64(np.float32(rec["after"])) / np.float64(np.float32(rec["before"]))))
            else:
                assert rec["shift"] == float(onset_shift(before, after, strength, 0.5)) == 1.0


def test_headline_shape_in_one_process(be):
    data = onset_workers.headline_data()
    out = onset_workers.folded_headline(0, 1)
    assert len(out) == 3
    for rep in out:
        _check_headline_gpu(rep, data)
        assert rep["tails"] == {}


@pytest.mark.parametrize("world,tail_quantile", [(2, 0.0), (4, 0.95)])
def test_headline_shape_on_processes_sharing_the_gpu(world, tail_quantile):
    """Default route (gloo / c10d); with four processes tail scores are on as well: two follow-up steps behind one report,
    each with its own all-gather."""
    data = onset_workers.headline_data()
    res = run_ranks(onset_workers.folded_headline, world, timeout=300, use_oracle_backend=False, device=0,
                    tail_quantile=tail_quantile)
    assert all(r == [None] * 3 for r in res[1:])
    for rep in res[0]:
        _check_headline_gpu(rep, data)
        assert bool(rep["tails"]) == bool(tail_quantile)
        if tail_quantile:
            assert rep["tails"]["quantile"] == tail_quantile and sorted(rep["tails"]["section_tails"]) == sorted(
                rep["onsets"]["section_onsets"])


@pytest.mark.parametrize("asynchronous", [False, True])
def test_next_window_written_from_another_stream_right_after_the_report(asynchronous):
    """The ordering rule: the onset kernel has read its window before the report call returns."""
    res = run_ranks(onset_workers.ring_windows_written_from_another_stream, 1, timeout=300, use_oracle_backend=False, device=0,
                    asynchronous=asynchronous)[0]
    samples, names, steps = res["samples"], res["names"], res["steps"]
    n = samples.shape[2]
    assert len(res["reports"]) == samples.shape[0] == 12
    for w, rep in enumerate(res["reports"]):
        for s, name in enumerate(names):
            rec = rep["section_onsets"][name]
            (ago, before, after, strength), _ = row_onset_one(samples[w, s], SEG_PPM)
            assert rec["samples_ago"] == int(ago) == n - int(steps[w, s]) and rec["window"] == n, (w, name, rec)
            assert abs(rec["before"] - float(before)) <= float(np.spacing(before)), (w, name, rec, before)
            assert abs(rec["after"] - float(after)) <= float(np.spacing(after)), (w, name, rec, after)
            assert abs(rec["strength"] - float(strength)) <= 1.2e-7 and abs(rec["shift"] - 1.5) < 0.01, (w, name, rec)
        # every section stepped by the same factor: one rank is its own reference
        assert all(v == 1.0 for v in rep["section_relative"].values())
        at_return, before_read, after_first, after_second = rep["copy_outs"]
        # neither the report call nor scores / stragglers copy onsets out; the first onset_scores() does, exactly once
        assert at_return == before_read == w and after_first == after_second == w + 1, (w, rep["copy_outs"])


def test_wrapped_ring_is_walked_in_time_order():
    """1.5 x ring_cap samples (and 2 x + 5) pushed into 64-deep rings with the step inside the surviving window, between
    windows that do not wrap."""
    res = run_ranks(onset_workers.wrapped_ring, 1, timeout=300, use_oracle_backend=False, device=0)[0]
    assert len(res["windows"]) == 4
    for w in res["windows"]:
        pushed = w["pushed"]
        n = min(pushed.shape[1], 64)
        for s, name in enumerate(res["names"]):
            rec = w["onsets"][name][0]
            (ago, before, after, strength), _ = row_onset_one(pushed[s, -n:], SEG_PPM)
            assert rec["samples_ago"] == int(ago) == 10 + 7 * s and rec["window"] == n, (name, rec)
            assert abs(rec["before"] - float(before)) <= float(np.spacing(before)), (name, rec, before)
            assert abs(rec["after"] - float(after)) <= float(np.spacing(after)), (name, rec, after)
            assert abs(rec["strength"] - float(strength)) <= 1.2e-7 and abs(rec["shift"] - 1.5) < 0.02, (name, rec)
