"""GPU parity of the stall kernel (``k_row_stall``), of ``nvrx_stall_score`` and of the stall step of a report against
``stall_ref`` below, a NumPy restatement of the definition in include/nvrx_straggler.h (``np.partition`` on the key-mapped
values, ``np.diff`` on the flags, f64 sums).

Bounds.  ``events``, ``samples``, ``last_ago`` and the bits of ``pace``, ``spread`` and ``cut``: exact.  ``level`` and ``share``
are f32 roundings of f64 sums whose order differs from NumPy's by at most n * 2^-53 = 7e-12 relative at n = 65 536, far below
half an f32 ulp: only a value on a rounding boundary can differ, by one ulp, which is the bound.  ``e`` is the stated function
of the record's own f32 fields, to the bit."""
import numpy as np
import pytest
import torch

from nvrx_straggler._native import STALL_LDS_SAMPLES as CUT
from tail_oracle_backend import tail_scores_table
from test_gpu_score import _random_table
from test_row_group_host import _example

pytestmark = pytest.mark.gpu

RATIO_PPM, MIN_Z, MIN_SHARE = 1500000, 6.0, 0.01
PAD, FILL = 64, 0x5A5A5A5A
KINDS = ("noise", "ends", "straddle", "two_runs", "constant", "slow_30", "one_nan", "one_inf")


@pytest.fixture(scope="module")
def be():
    from nvrx_straggler.backend import get_backend

    return get_backend()


def _row(kind, rng, n):
    """One row of ``n`` samples around 1000 with 1 % noise; stall samples are 50 x."""
    x, at = 1000.0 * (1.0 + 0.01 * rng.standard_normal(n)), []
    if kind == "ends":
        at = [0, n - 1]
    elif kind == "straddle":  # runs of two across, from and up to every 64-sample boundary (256 and the waves' spans among them)
        at = [b + d for j, b in enumerate(range(64, n, 64)) for d in ((-1, 0), (0, 1), (-2, -1))[j % 3]]
    elif kind == "two_runs":
        at = [n // 2 + d for d in (0, 1, 3, 4, 5)]
    elif kind == "constant":
        x[:] = 1234.5
    elif kind == "slow_30":
        x[rng.random(n) < 0.3] *= 3.0
    elif kind == "one_nan":
        x[n // 2] = np.nan
    elif kind == "one_inf":
        x[n // 3] = np.inf
    x[[i for i in at if 0 <= i < n]] *= 50.0
    return x.astype(np.float32)


def _lower_median(a):
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    keys = np.where(u >> 31, ~u, u | np.uint32(0x80000000))  # f2key
    k = (500000 * a.size + 999999) // 1000000 - 1
    key = np.partition(keys, k)[k]
    return np.array([key ^ np.uint32(0x80000000) if key >> 31 else ~key], dtype=np.uint32).view(np.float32)[0]


def stall_ref(x, n, start=0):
    """``((events, samples, last_ago), (pace, spread, cut, level, share))`` of one row; level and share as f64."""
    n = min(int(n), len(x))
    if n == 0:
        return (0, 0, 0), (-1.0,) * 5
    with np.errstate(all="ignore"):
        x = np.roll(np.asarray(x[:n], dtype=np.float32), -(int(start) % n))  # time order
        pace = _lower_median(x)
        spread = _lower_median(np.abs(x - pace))
        p = np.float64(pace)
        cut = np.float32(np.fmax(p * RATIO_PPM / 1e6, p + np.float64(MIN_Z) * 1.4826 * np.float64(spread)))
        f = x > cut
        T, lost = x.astype(np.float64).sum(), (x[f].astype(np.float64) - p).sum()
        if not (np.isfinite(T) and np.isfinite(lost)):
            return (0, 0, 0), (np.nan,) * 5
        if n < 8 or not f.any():
            return (0, 0, 0), (pace, spread, cut, pace, 0.0)
        events = int(f[0]) + int((np.diff(f.astype(np.int8)) == 1).sum())
        return (events, int(f.sum()), n - 1 - int(np.flatnonzero(f)[-1])), (pace, spread, cut, p + lost / f.sum(), lost / T)


def stall_excess(events, pace, level, share, min_share=MIN_SHARE):
    pace, level = np.float32(pace), np.float32(level)
    if events >= 1 and np.float32(share) >= np.float32(min_share) and level > pace > 0:
        return np.float32(np.float64(level) / np.float64(pace))
    return np.float32(1.0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _within_ulp(got, want):
    want = np.float32(want)
    return abs(float(got) - float(want)) <= float(np.spacing(np.abs(want)))


def _stall(be, samples, counts, starts=None):
    """``nvrx_row_stall`` into a guard-padded buffer -> ``[rows, 8]`` uint32 words."""
    rows, stride = samples.shape
    s = torch.from_numpy(np.ascontiguousarray(samples, dtype=np.float32)).cuda()
    c = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int32)).cuda()
    st = None if starts is None else torch.from_numpy(np.ascontiguousarray(starts, dtype=np.int32)).cuda()
    big = torch.full((PAD + rows * 8 + PAD,), FILL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = be.lib.nvrx_row_stall(s.data_ptr(), c.data_ptr(), None if st is None else st.data_ptr(), rows, stride, RATIO_PPM, MIN_Z,
                               big[PAD:].data_ptr(), be.stream_handle)
    assert rc == 0, be.lib.nvrx_last_error()
    be.synchronize()
    host = big.cpu().numpy().view(np.uint32)
    assert (host[:PAD] == FILL).all() and (host[PAD + rows * 8 :] == FILL).all(), "outside the records"
    return host[PAD : PAD + rows * 8].reshape(rows, 8).copy()


def _check(rec, x, n, where, start=0):
    (events, samples, last_ago), vals = stall_ref(x, n, start)
    got = rec[3:].view(np.float32)
    assert tuple(rec[:3]) == (events, samples, last_ago), (where, rec, events, samples, last_ago)
    if np.isnan(vals[0]):
        assert np.isnan(got).all(), (where, got)
        return
    assert np.array_equal(rec[3:6], _bits(vals[:3])), (where, got, vals)
    assert _within_ulp(got[3], vals[3]) and _within_ulp(got[4], vals[4]), (where, got, vals)


@pytest.mark.parametrize("n,stride", [(0, 8), (7, 8), (8, 8), (9, 12), (255, 256), (256, 256), (257, 260), (1025, 1028),
                                      (4096, 4096), (4100, 4100), (CUT, CUT), (CUT + 4, CUT + 4), (65536, 65536)])
def test_row_stall_every_size_and_data_kind(be, n, stride):
    """Rows of every kind at the sizes where a mechanism changes: the record's floor, whole and partial steps, more than one
    step a wave, the 256- and the 1024-thread variant, rows inside and beyond the staging buffer, the longest ring."""
    rng = np.random.default_rng(n)
    rows = np.stack([np.resize(_row(kind, rng, n), stride) if n else np.zeros(stride, np.float32) for kind in KINDS])
    rec = _stall(be, rows, np.full(len(KINDS), n, dtype=np.uint32))
    for r, kind in enumerate(KINDS):
        _check(rec[r], rows[r], n, (kind, n))
    if n >= 256:
        by_kind = {kind: stall_ref(rows[r], n) for r, kind in enumerate(KINDS)}
        assert by_kind["straddle"][0][0] == (n - 1) // 64 and by_kind["constant"][1][1:3] == (0.0, np.float32(1234.5 * 1.5))
        assert by_kind["slow_30"][0][1] > n // 5 and by_kind["slow_30"][1][1] > 0.0  # (a third of the row is not swallowed)
    if n == 1025:  # the backend's operator returns the same words
        s, c = torch.from_numpy(rows).cuda(), torch.full((len(KINDS),), n, dtype=torch.int32, device="cuda")
        assert np.array_equal(be.row_stall(s, c, RATIO_PPM, MIN_Z).cpu().numpy().view(np.uint32), rec)


@pytest.mark.parametrize("n", [1000, 10000, 20000])
def test_row_stall_ring_starts(be, n):
    """A ring with a run in slots 100 .. 104 and stalls in slots 0 and n - 1, read from the run's first slot, from inside it and
    from elsewhere: a run across the physical wrap is one event, a run cut by the window's ends two; words as un-rotated."""
    x = _row("noise", np.random.default_rng(n), n)
    x[[0, 100, 101, 102, 103, 104, n - 1]] *= np.float32(50.0)
    starts = np.array([0, 100, 102, 105, n // 2, n - 1], dtype=np.uint32)
    rec = _stall(be, np.stack([x] * len(starts)), np.full(len(starts), n, dtype=np.uint32), starts)
    flat = _stall(be, np.stack([np.roll(x, -int(s)) for s in starts]), np.full(len(starts), n, dtype=np.uint32))
    assert np.array_equal(rec, flat)  # (the sums' order follows the time index: also level and share, to the bit)
    for r, s in enumerate(starts):
        _check(rec[r], x, n, ("start", n, int(s)), start=s)
    assert [int(e) for e in rec[:, 0]] == [3, 2, 3, 2, 2, 2] and (rec[:, 1] == 7).all()


def test_stall_score_matches_numpy(be):
    """``nvrx_stall_score`` on a random 7-plane table: the tail oracle on plane 0; the planes come back unchanged."""
    R, K, S = 65, 7, 3
    rng = np.random.default_rng(11)
    T = _random_table(rng, R, K, S)
    have = rng.random((R, K + S)) >= 0.15
    have[:, :3], have[:, K + S - 1] = True, True  # three kernels and a section that nobody misses
    planes = np.where(have[:, None, :], rng.uniform(0.0, 100.0, (R, 7, K + S)), -1.0).astype(np.float32)
    planes[:, 0, :] = np.where(have, np.where(rng.random((R, K + S)) < 0.5, 1.0, rng.uniform(1.0, 60.0, (R, K + S))), -1.0)
    ws = be.workspace(R, K, S, R, 0)
    ws.stall_settle()
    ws.send.copy_(torch.from_numpy(T))
    _, table, _, _ = ws.stall_buffers()
    table.copy_(torch.from_numpy(planes.reshape(R, -1)))
    torch.cuda.synchronize()
    got_planes, got = be.stall_score(ws, table, ws.send).records()
    exp = tail_scores_table(planes[:, 0, :], T, K, S)
    assert np.array_equal(_bits(got_planes), _bits(planes))
    assert got.shape == exp.shape == (R, 1 + S) and np.array_equal(np.isnan(got), np.isnan(exp))
    ok = ~np.isnan(exp[:, 1:])
    assert np.array_equal(_bits(got[:, 1:][ok]), _bits(exp[:, 1:][ok]))  # one f64 quotient rounded to f32
    ok = np.isfinite(exp[:, 0])
    assert ok.all() and np.abs(got[ok, 0].astype(np.float64) - exp[ok, 0].astype(np.float64)).max() <= 2e-6  # (f32 weights, an f32 result)


def test_stall_local_planes(be):
    """2 logical ranks x 3 sections of 600 samples from rings, rank 1 without its last section: the report's planes and a
    second, guard-padded ``nvrx_stall_local`` on the same window -- every slot written, -1 where no row has the id, the
    restatement's values elsewhere, ``e`` the stated function of the planes."""
    from nvrx_straggler.folded import FoldedJob

    rng = np.random.default_rng(3)
    kinds = (("noise", "ends", "straddle"), ("two_runs", "slow_30"))
    data = [[_row(kind, rng, 600) for kind in per] for per in kinds]
    job = FoldedJob(total_ranks=2, sections=3, ring_cap=600, scores_to_compute=("relative_perf_scores",), stall_detection=True,
                    stall_min_ratio=RATIO_PPM / 1e6, stall_min_z=MIN_Z, stall_min_share=MIN_SHARE)
    try:
        for lr, per in enumerate(data):
            for s, x in enumerate(per):
                job.rings.push_device(job.rows[job.section_names[s]], torch.from_numpy(x).cuda(), lr=lr)
        job.backend.synchronize()
        rep = job.report(reset=False)
        src = rep.__dict__["_stall"]
        K, S, ids = src.handle.K, src.handle.S, dict(src.sections)
        planes, _ = src.handle.records()
        big = torch.full((PAD + 2 * 7 * (K + S) + PAD,), np.float32(FILL), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        rc = be.lib.nvrx_stall_local(job.rings.ctx, None, RATIO_PPM, MIN_Z, MIN_SHARE, big[PAD:].data_ptr(), K, S, 0, be.stream_handle)
        assert rc == 0, be.lib.nvrx_last_error()
        be.synchronize()
        scores = rep.stall_scores()
    finally:
        job.close()
    host = big.cpu().numpy()
    assert (host[:PAD] == np.float32(FILL)).all() and (host[PAD + planes.size :] == np.float32(FILL)).all(), "outside the planes"
    assert np.array_equal(_bits(host[PAD : PAD + planes.size]), _bits(planes).ravel())
    planes = planes.reshape(2, 7, K + S)
    expected = np.full((2, 7, K + S), -1.0)
    for lr, per in enumerate(data):
        for s, x in enumerate(per):
            col = K + ids[job.section_names[s]]
            (events, _, ago), (pace, _, _, level, share) = stall_ref(x, 600)
            e, got = planes[lr, 0, col], planes[lr, :, col]
            assert e == stall_excess(int(got[4]), got[1], got[2], got[3]), (lr, s, got)
            assert _within_ulp(got[2], level) and _within_ulp(got[3], share), (lr, s, got, level, share)
            expected[lr, :, col] = (e, pace, got[2], got[3], events, ago, 600)
    assert np.array_equal(planes, expected.astype(np.float32))
    assert planes[1, 0, K + ids[job.section_names[0]]] > 40.0 and planes[0, 0, K + ids[job.section_names[0]]] == 1.0
    assert set(scores["section_stalls"][job.section_names[2]]) == {0} and scores["min_share"] == MIN_SHARE


@pytest.mark.parametrize("grouped", [False, True])
def test_the_example_job_end_to_end(be, grouped):
    """The job of ``examples/straggler_example.py --stall`` with every row family on: ten stalls of 50 x among 10 000 samples
    are named by the stall scores alone (rank 5), one stall (rank 2) by nobody; with ``row_peer_groups`` too."""
    from nvrx_straggler.folded import FoldedJob

    ex = _example()
    x = ex.stall_samples().astype(np.float32)
    job = FoldedJob(total_ranks=8, sections=2, ring_cap=10000, scores_to_compute=("relative_perf_scores",), **ex.STALL_OPTIONS,
                    **({"row_peer_groups": True, "peer_groups": "block:4"} if grouped else {}))
    try:
        for r in range(8):
            job.load(r, x[r])
        rep = job.report()
        stalls, tails, found = rep.stall_scores(), rep.tail_scores(), ex.named_ranks(rep.identify_stall_stragglers())
        others = {f: ex.named_ranks(getattr(rep, f"identify_{f}_stragglers")()) for f in ex.STALL_FAMILIES[:-1]}
        others["relative"] = ex.named_ranks({k: v for k, v in rep.identify_stragglers().items() if "relative" in k})
        relative = rep.section_relative_perf_scores
    finally:
        job.close()
    assert found == [5], found
    for s, name in enumerate(job.section_names):
        (events, _, ago), (pace, _, _, level, share) = stall_ref(x[5, s], 10000)
        rec = stalls["section_stalls"][name][5]
        assert (rec["events"], rec["last_samples_ago"], rec["window"], events) == (10, ago, 10000, 10), (name, rec)
        assert _within_ulp(rec["share"], share) and _within_ulp(rec["level"], level) and rec["pace"] == float(pace), (name, rec)
        assert rec["excess"] == float(stall_excess(10, rec["pace"], rec["level"], rec["share"])) and rec["excess"] > 40.0, (name, rec)
        assert stalls["section_stalls"][name][2]["excess"] == 1.0 and stalls["section_stalls"][name][2]["events"] == 1
        if not grouped:  # (job-wide references: order statistics that ten samples cannot move beyond the 1 % noise)
            assert relative[name][5] >= 0.99 and tails["section_relative"][name][5] >= 0.99, (name, relative[name], tails)
    assert others == {f: [] for f in others}, others
