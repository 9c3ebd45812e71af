"""GPU parity of the ramp kernels (``k_row_ramp``, ``k_tail_score`` on the ramp planes) and of the ramp step of a report against
``ramp_ref`` below: a NumPy f64 restatement of the definition in include/nvrx_straggler.h (cumsum, the closed forms, argmax
over the full R_t curve).

Bounds.  A priori: f64 roundoff is 1.1e-16, times 65 536 additions that is 7e-12 relative on a prefix sum, for C_t and for the
index-weighted V_t alike (relative to sum |i * d_i|); Shd = (W - V_t) - t * (T - C_t) cancels by (n / L)^2, 400 x at the
shortest rising part of 5 %, and R squares it: 6e-9 at worst, inside 1e-8, so the index weight is not re-centred.  Measured on
the CPU, on this file's own rows at n = 65 536 (every kind of ``KINDS``, the rows of both stride-65536 tests): the f64
restatement differs from the same formulas in ``np.longdouble`` by at most 1.6e-13 on any strength of any curve (hinge_30;
below 2e-15 on every other row -- the pivoted f32 samples are multiples of 2^-14, so the sums of d are exact in f64 in any
order and those of i * d nearly so).  TOL = 8 x 1.6e-13 = 1.3e-12: the margin is for the kernel's different summation order.  The record
carries the strength as f32: it is compared with the restatement's f64 strength within TOL plus half an f32 ulp at that
value.  ``base`` / ``end``: within one f32 ulp where t* agrees.  The knot: the restatement's strength at the kernel's t* is
within TOL of its maximum, and wherever its runner-up is further below the maximum than that, t* is equal.  Absent, short,
constant and non-finite rows are compared exactly."""
import numpy as np
import pytest
import torch

from nvrx_straggler._native import RAMP_LDS_SAMPLES as CUT
from row_group_oracle_backend import row_group_records
from tail_oracle_backend import tail_scores_table
from test_gpu_score import _random_table

pytestmark = pytest.mark.gpu

SEG_PPM = 50000
TOL = 1.3e-12
KINDS = ("noise", "line", "hinge_30", "hinge_70", "hinge_95", "falling", "step", "constant", "one_nan", "one_inf")


@pytest.fixture(scope="module")
def be():
    from nvrx_straggler.backend import get_backend

    return get_backend()


def _row(kind, rng, n):
    """One row of ``n`` samples around 1000 with 1 % noise."""
    x, i = 1000.0 * (1.0 + 0.01 * rng.standard_normal(n)), np.arange(n)
    if kind == "line":
        x += i * (300.0 / max(n, 1))
    elif kind.startswith("hinge_"):
        t = int(n * int(kind[6:]) / 100)
        x += np.maximum(0, i - t) * (500.0 / max(n - t, 1))
    elif kind == "falling":
        x -= np.maximum(0, i - n // 2) * (400.0 / max(n, 1))
    elif kind == "step":
        x[int(0.7 * n):] *= 1.5
    elif kind == "constant":
        x[:] = 1234.5
    elif kind == "one_nan":
        x[n // 2] = np.nan
    elif kind == "one_inf":
        x[n // 3] = np.inf
    return x.astype(np.float32)


def ramp_ref(x, n, seg_ppm=SEG_PPM, start=0, dtype=np.float64):
    """``((ago, base, end, strength), curve)`` of one row: the record in ``dtype``, and R_t / SST at every knot t = 0 .. n - m
    (None for an absent, non-finite, short or constant row)."""
    n = min(int(n), len(x))
    if n == 0:
        return (0, -1.0, -1.0, -1.0), None
    with np.errstate(all="ignore"):
        x = np.roll(np.asarray(x[:n]), -(int(start) % n)).astype(dtype)  # time order
        d, i, nd = x - x[0], np.arange(n).astype(dtype), dtype(n)
        C, V = np.concatenate(([0], np.cumsum(d))), np.concatenate(([0], np.cumsum(i * d)))
        T, W = C[-1], V[-1]
        SST = ((d - T / nd) ** 2).sum()
        if not (np.isfinite(T) and np.isfinite(W) and np.isfinite(SST)):
            return (0, np.nan, np.nan, np.nan), None
        m = max(8, (seg_ppm * n + 999999) // 1000000)
        if n < 2 * m:
            return (0, x[0] + T / nd, x[0] + T / nd, 0.0), None
        if SST == 0:
            return (n, x[0], x[0], 0.0), None
        t = np.arange(n - m + 1).astype(dtype)
        L = nd - t
        Sh, Shh = L * (L - 1) / 2, (L - 1) * L * (2 * L - 1) / 6
        Shd = (W - V[: n - m + 1]) - t * (T - C[: n - m + 1])
        Shd_c, Shh_c = Shd - Sh * T / nd, Shh - Sh * Sh / nd
        curve = Shd_c * Shd_c / Shh_c / SST
        k = int(np.argmax(curve))  # (the first of equals)
        b = Shd_c[k] / Shh_c[k]
        base = x[0] + (T - b * Sh[k]) / nd
        return (n - k, base, base + b * (L[k] - 1), curve[k]), curve


def ramp_rise(base, end, strength, min_strength):
    base, end, strength = np.float32(base), np.float32(end), np.float32(strength)
    if strength >= np.float32(min_strength) and end > base > 0:
        return np.float32(np.float64(end) / np.float64(base))
    return np.float32(1.0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _ramp(be, samples, counts, starts=None):
    s = torch.from_numpy(np.ascontiguousarray(samples, dtype=np.float32)).cuda()
    c = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int32)).cuda()
    st = None if starts is None else torch.from_numpy(np.ascontiguousarray(starts, dtype=np.int32)).cuda()
    rec = np.ascontiguousarray(be.row_ramp(s, c, SEG_PPM, st).cpu().numpy()).view(np.uint32)
    return rec[:, 0].copy(), rec[:, 1:].copy().view(np.float32)


def _ulps(got, want):
    return abs(float(got) - float(want)) / float(np.spacing(np.abs(np.float32(want))))


def _check(be, samples, counts, tag, starts=None):
    ago, vals = _ramp(be, samples, counts, starts)
    worst = {"at_knot": 0.0, "strength": 0.0, "ulp": 0.0}
    for r in range(samples.shape[0]):
        n = min(int(counts[r]), samples.shape[1])
        exp, curve = ramp_ref(samples[r], n, start=0 if starts is None else starts[r])
        got = (int(ago[r]), *vals[r])
        where = (tag, r, n, got, exp)
        if curve is None:  # absent, non-finite, short or constant: exact (NaN by NaN-ness)
            assert got[0] == exp[0], where
            if np.isnan(exp[3]):
                assert np.isnan(vals[r]).all(), where
            else:
                assert np.array_equal(_bits(vals[r]), _bits(exp[1:])), where
            continue
        t_got, best = n - got[0], int(np.argmax(curve))
        top = float(curve[best])
        assert 0 <= t_got < curve.size, where
        at_knot = top - float(curve[t_got])
        runner_up = float(np.max(np.delete(curve, best)))
        d = max(0.0, abs(float(got[3]) - top) - 0.5 * float(np.spacing(np.float32(top))))
        worst["at_knot"], worst["strength"] = max(worst["at_knot"], at_knot), max(worst["strength"], d)
        assert at_knot <= TOL, where + (at_knot,)
        if top - runner_up > TOL:
            assert t_got == best, where + (top - runner_up,)
        assert d <= TOL, where + (d,)
        if t_got == best:
            u = max(_ulps(got[1], exp[1]), _ulps(got[2], exp[2]))
            worst["ulp"] = max(worst["ulp"], u)
            assert u <= 1.0, where + (u,)
    print(f"{tag}: worst {worst}")
    return ago, vals


@pytest.mark.parametrize("stride", [8, 64, 256, 1000, 4100, 10000, CUT, CUT + 4, 65536])
def test_row_ramp_every_stride_count_and_data_kind(be, stride):
    """Every data kind at every count: 70 rows per launch, both launch variants and both staging paths."""
    rng = np.random.default_rng(stride)
    rows, counts = [], []
    for kind in KINDS:
        for c in (0, 1, 15, 16, 17, 33, stride):
            rows.append(_row(kind, rng, stride))
            counts.append(min(c, stride))
    _check(be, np.stack(rows), np.array(counts, dtype=np.uint32), ("stride", stride))


@pytest.mark.parametrize("stride", [64, 1000, 65536])
def test_row_ramp_ring_starts(be, stride):
    """Full rows whose oldest sample lives in slot 0, 1, 3, n/2 and n-1: the rotated rows give the records of the unrotated ones."""
    rng = np.random.default_rng(stride + 1)
    rows, starts = [], []
    for kind in KINDS:
        x = _row(kind, rng, stride)
        for start in (0, 1, 3, stride // 2, stride - 1):
            rows.append(np.roll(x, start))
            starts.append(start)
    ago, vals = _check(be, np.stack(rows), np.full(len(rows), stride, dtype=np.uint32), ("starts", stride),
                       starts=np.array(starts, dtype=np.uint32))
    for b in range(0, len(rows), 5):  # the same samples in time order: the very same arithmetic
        assert (ago[b : b + 5] == ago[b]).all(), (stride, b, ago[b : b + 5])
        assert all(np.array_equal(_bits(vals[b + j]), _bits(vals[b])) or np.isnan(vals[b]).all() for j in range(1, 5)), (stride, b)


@pytest.mark.parametrize("R,K,S,grouped", [(1, 0, 1, False), (3, 5, 2, False), (65, 7, 3, True)])
def test_ramp_score_matches_numpy(be, R, K, S, grouped):
    """``nvrx_ramp_score`` on a random table: ref / e per section to the bit, the weighted GPU mean in f64 within 2e-6 (f32
    weights and an f32 result); ``grouped``: through ``ramp_group_score`` with two groups as well."""
    rng = np.random.default_rng(R * 1000 + K + S)
    KS = K + S
    T = _random_table(rng, R, K, S)
    have = rng.random((R, KS)) >= 0.15
    have[:, KS - 1] = True  # a column nobody misses
    planes = np.where(have[:, None, :], rng.uniform(0.0, 100.0, (R, 6, KS)), -1.0).astype(np.float32)
    planes[:, 0, :] = np.where(have, np.where(rng.random((R, KS)) < 0.5, 1.0, rng.uniform(1.0, 3.0, (R, KS))), -1.0)
    ws = be.workspace(R, K, S, R, 0)
    ws.ramp_settle()
    ws.send.copy_(torch.from_numpy(T))
    _, table, _, _ = ws.ramp_buffers()
    table.copy_(torch.from_numpy(planes.reshape(R, -1)))
    torch.cuda.synchronize()

    def compare(got, exp):
        assert got.shape == exp.shape == (R, 1 + S) and np.array_equal(np.isnan(got), np.isnan(exp))
        ok = ~np.isnan(exp[:, 1:])
        assert np.array_equal(_bits(got[:, 1:][ok]), _bits(exp[:, 1:][ok]))  # one f64 quotient rounded to f32
        ok = np.isfinite(exp[:, 0])
        assert not ok.any() or np.abs(got[ok, 0].astype(np.float64) - exp[ok, 0].astype(np.float64)).max() <= 2e-6

    got_planes, scores = be.ramp_score(ws, table, ws.send).records()
    assert np.array_equal(_bits(got_planes), _bits(planes))
    compare(scores, tail_scores_table(planes[:, 0, :], T, K, S))
    if grouped:
        from nvrx_straggler.backend import PeerGroups

        groups = PeerGroups([r % 2 for r in range(R)])
        _, table, _, _ = ws.ramp_buffers()
        got_planes, scores, _ = be.ramp_group_score(ws, table, ws.send, groups, 0, R, 2).records()
        assert np.array_equal(_bits(got_planes), _bits(planes))
        compare(scores, row_group_records(planes[:, 0, :], T, K, S, groups.host, groups.G, 0, R, 2)[1])


def test_one_report_end_to_end(be):
    """4 folded ranks x (3 sections + 1 kernel) x 1000 samples from rings, rank 2 with a hinge 60 % into every row's window."""
    from nvrx_straggler.folded import FoldedJob

    RANKS, SECTIONS, N, SLOW, MIN_STRENGTH = 4, 3, 1000, 2, 0.5
    rng = np.random.default_rng(5)
    data = (1000.0 * (1.0 + 0.01 * rng.standard_normal((RANKS, SECTIONS, N)))).astype(np.float32)
    data[SLOW] += (np.maximum(0, np.arange(N) - 600) * (500.0 / 400.0)).astype(np.float32)
    reports = {}
    for on in (True, False):
        job = FoldedJob(total_ranks=RANKS, sections=SECTIONS, ring_cap=N, scores_to_compute=("relative_perf_scores",),
                        kernel_names=("gemm",), ramp_detection=on, ramp_min_segment=SEG_PPM / 1e6,
                        ramp_min_strength=MIN_STRENGTH)
        try:
            for r in range(RANKS):
                job.load(r, data[r])
                job.load_kernels(r, data[r, :1])  # (the kernel row holds section 0's samples)
            rep = reports[on] = job.report()
            scores, found = rep.ramp_scores(), rep.identify_ramp_stragglers()
            names = job.section_names
        finally:
            job.close()
    assert "_ramp" not in reports[False].__dict__ and scores == {} and found["straggler_gpus_relative"] == set()
    rep = reports[True]
    scores, found = rep.ramp_scores(), rep.identify_ramp_stragglers()
    assert (scores["min_segment"], scores["min_strength"]) == (SEG_PPM / 1e6, MIN_STRENGTH)
    assert scores["kernel_ramps"] == {"gemm": scores["section_ramps"][names[0]]}
    rises = np.ones((RANKS, SECTIONS), dtype=np.float32)
    for s, name in enumerate(names):
        for r in range(RANKS):
            (ago, base, end, strength), _ = ramp_ref(data[r, s], N)
            rec = scores["section_ramps"][name][r]
            rises[r, s] = ramp_rise(base, end, strength, MIN_STRENGTH)
            assert (rec["samples_ago"], rec["window"], rec["whole_window"]) == (ago, N, ago == N), (name, r, rec, ago)
            assert _ulps(rec["base"], base) <= 1.0 and _ulps(rec["end"], end) <= 1.0, (name, r, rec, base, end)
            assert abs(rec["strength"] - float(strength)) <= TOL + 0.5 * float(np.spacing(np.float32(strength))), (name, r, rec)
            assert rec["rise"] == float(ramp_rise(rec["base"], rec["end"], rec["strength"], MIN_STRENGTH)), (name, r, rec)
            if r == SLOW:
                assert abs(ago - 400) <= 10 and 1.45 < rec["rise"] < 1.55 and rec["strength"] > 0.9, (name, rec)
    assert (rises[SLOW] > 1.4).all() and (np.delete(rises, SLOW, axis=0) == 1.0).all()
    for s, name in enumerate(names):  # one f64 quotient rounded to f32, from the records' own rises
        e = [scores["section_ramps"][name][r]["rise"] for r in range(RANKS)]
        assert [scores["section_relative"][name][r] for r in range(RANKS)] == [
            float(np.float32(np.float64(np.float32(min(e))) / np.float64(np.float32(x)))) for x in e], name
    for r in range(RANKS):  # (one kernel: the weighted mean is its quotient, through one more f64 product and quotient)
        assert abs(scores["gpu_relative"][r] - scores["section_relative"][names[0]][r]) <= 2e-6, (r, scores["gpu_relative"])
    assert {s.rank for s in found["straggler_gpus_relative"]} == {SLOW}
    assert {n: {s.rank for s in ids} for n, ids in found["straggler_sections_relative"].items()} == {n: {SLOW} for n in names}
