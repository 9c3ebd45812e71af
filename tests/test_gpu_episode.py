"""GPU parity of the episode kernels (``k_row_episode``, ``k_tail_score`` on the episode planes) and of the episode step of a
report against the NumPy restatement of tests/episode_oracle_backend.py.  Every row of every case is compared.

Bounds (include/nvrx_straggler.h has the definition), by the onset test's own argument.  The kernel and NumPy add the same f64
numbers in different orders: f64 roundoff is 1.1e-16, times 65 536 additions that is 7e-12 relative to A = sum |d_i| on a
prefix C_t.  E = (H_b - H_a) / n = (C_b - C_a) - (b - a) * T / n takes two prefixes and a share of the total: at most about
1.5e-11 * A in the worst case, and 1e-10 * A leaves about 7 x.
  E          the oracle's E at the kernel's (a, b) is within 1e-10 * A of the oracle's largest; a kernel that reports no
             episode has an oracle maximum of at most that;
  (a, b)     equal to the oracle's wherever every other b of the oracle's curve M_b = max_a E lies further below the largest
             than 1e-10 * A, the largest further from 0 than that, and the second-smallest admissible H_a of the winning b
             further above the smallest than that (in units of E); no more than 2 % of a case's rows may lie inside that
             band (tests/test_episode_host.py checks that on the oracle alone; the expected count is zero).  On every
             planted-stretch row and every integer-valued row (exact sums: ties are decided bit for bit, the lowest b, then
             the lowest a) the interval is the oracle's unconditionally;
  strength   the record's f32 within 1e-9 plus half an f32 ulp of the oracle's f64 value at the kernel's (a, b): E squared
             doubles the relative 1e-10 / (E / A), E / A is at least a few percent wherever the strength is not negligible,
             and 1e-9 absolute on a value of at most 1 leaves room;
  inside / outside   within one f32 ulp where the interval agrees (an f64 sum rounded once to f32).
Absent, short, constant and non-finite rows are compared exactly: NaN by NaN-ness, the mean of a short row within one f32 ulp
(it is x_0 + T / n with T summed in another order) and bit for bit where the samples are integers."""
import numpy as np
import pytest
import torch

import episode_workers
from episode_oracle_backend import episode_excess, episode_one, episode_scores_table, row_episode, unpack_records
from test_gpu_score import _random_table

pytestmark = pytest.mark.gpu

_worst = {"excess_over_A": 0.0, "strength": 0.0, "strength_beyond_half_ulp": 0.0, "ulp": 0.0, "band_rows": 0, "rows": 0}
INTEGER_KINDS = ("two_equal", "int_noise", "constant")


@pytest.fixture(scope="module")
def be():
    from nvrx_straggler.backend import get_backend

    return get_backend()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _episode(be, samples, counts, len_ppm, starts=None):
    s = torch.from_numpy(np.ascontiguousarray(samples, dtype=np.float32)).cuda()
    c = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int32)).cuda()
    st = None if starts is None else torch.from_numpy(np.ascontiguousarray(starts, dtype=np.int32)).cuda()
    return unpack_records(be.row_episode(s, c, len_ppm, st).cpu().numpy())


def _within_one_ulp(got, want):
    d = abs(float(got) - float(want)) / float(np.spacing(np.abs(np.float32(want))))
    _worst["ulp"] = max(_worst["ulp"], d)
    return d <= 1.0


def _check(be, samples, counts, len_ppm, kinds, tag, starts=None):
    got_all = _episode(be, samples, counts, len_ppm, starts)
    exp, eps = row_episode(samples, counts, len_ppm, starts)
    band = set(episode_workers.band_rows(eps, kinds))
    _worst["band_rows"] = max(_worst["band_rows"], len(band))
    _worst["rows"] += samples.shape[0]
    assert len(band) <= 0.02 * samples.shape[0], (tag, sorted(band))
    for r in range(samples.shape[0]):
        n = min(int(counts[r]), samples.shape[1])
        g, e, ep = got_all[r], exp[r], eps[r]
        where = (tag, r, kinds[r], n, g, e)
        if ep is None or ep.M is None:
            # absent, non-finite or shorter than 3m: exact (NaN by NaN-ness)
            assert g["ago"] == 0 and g["length"] == 0, where
            if np.isnan(e["strength"]):
                assert np.isnan(g["inside"]) and np.isnan(g["outside"]) and np.isnan(g["strength"]), where
            else:
                assert _bits(g["strength"]) == _bits(e["strength"]) and _bits(g["inside"]) == _bits(g["outside"]), where
                if n == 0 or kinds[r] in INTEGER_KINDS:
                    assert _bits(g["inside"]) == _bits(e["inside"]), where
                else:
                    assert _within_one_ulp(g["inside"], e["inside"]), where
            continue
        tol = episode_workers.band_tol(ep)
        top = float(ep.M.max())
        pinned = r not in band or kinds[r] in episode_workers.EXACT_KINDS
        L = int(g["length"])
        if L == 0:  # the kernel found no episode: no interval lies above the row's mean
            assert top <= tol and g["ago"] == 0 and g["strength"] == 0.0 and _bits(g["inside"]) == _bits(g["outside"]), where + (top,)
            if pinned:
                assert ep.b == 0, where + (ep.a, ep.b)
            if ep.b == 0:
                assert _bits(g["inside"]) == _bits(e["inside"]) if kinds[r] in INTEGER_KINDS else _within_one_ulp(g["inside"], e["inside"]), where
            continue
        b = n - int(g["ago"])
        a = b - L
        assert ep.admissible(a, b), where + (a, b, ep.m)
        at = float(ep.e_at(a, b))
        if ep.A > 0:
            _worst["excess_over_A"] = max(_worst["excess_over_A"], (top - at) / ep.A)
        assert at >= top - tol and at > -tol, where + (a, b, at, top, tol)
        if pinned:
            assert (a, b) == (ep.a, ep.b), where + (a, b, ep.a, ep.b)
        s64 = at * at * n / (float(L) * float(n - L)) / ep.sst
        d = abs(float(g["strength"]) - s64)
        half_ulp = 0.5 * float(np.spacing(np.float32(s64)))
        _worst["strength"] = max(_worst["strength"], d)
        _worst["strength_beyond_half_ulp"] = max(_worst["strength_beyond_half_ulp"], max(0.0, d - half_ulp))
        assert d <= 1e-9 + half_ulp, where + (s64, d)
        if (a, b) == (ep.a, ep.b):
            if kinds[r] in INTEGER_KINDS:
                assert _bits(g["inside"]) == _bits(e["inside"]) and _bits(g["outside"]) == _bits(e["outside"]), where
            else:
                assert _within_one_ulp(g["inside"], e["inside"]) and _within_one_ulp(g["outside"], e["outside"]), where
        if kinds[r] == "two_equal":  # the exact tie goes to the first of the two stretches
            first = episode_workers.two_equal_first(n, ep.m)
            if first:
                assert (a, b) == first, where + (a, b, first)
    return got_all


@pytest.mark.parametrize("len_ppm", episode_workers.PPMS)
@pytest.mark.parametrize("stride", episode_workers.STRIDES)
def test_row_episode_every_stride_count_and_data_kind(be, stride, len_ppm):
    """Every data kind at every count: strides 4 .. 65 536, either side of the 256-thread / 1024-thread boundary (4096 / 4100),
    minimum lengths whose lag stays inside a wave's span, crosses 256-sample blocks (5000 ppm at 65 536: m = 328) and crosses
    wave spans (333 333 ppm: m = n / 3)."""
    samples, counts, kinds = episode_workers.kernel_case(stride, len_ppm)
    _check(be, samples, counts, len_ppm, kinds, ("stride", stride, len_ppm))
    print(f"stride {stride} ppm {len_ppm}: {samples.shape[0]} rows, worst so far {_worst}")


@pytest.mark.parametrize("stride", episode_workers.ROTATION_STRIDES)
def test_row_episode_ring_starts(be, stride):
    """Full rows whose oldest sample lives in slot 0, 1, 3, n/2 and n-1: the rotated rows give the records of the unrotated
    ones, bit for bit, and the same bits from launch to launch."""
    samples, counts, starts, kinds = episode_workers.rotation_case(stride)
    got = _check(be, samples, counts, episode_workers.LEN_PPM, kinds, ("starts", stride), starts=starts)
    raw = got.view(np.uint8).reshape(got.shape[0], -1)
    for base in range(0, samples.shape[0], 5):  # the same samples in time order: the very same arithmetic
        assert all(np.array_equal(raw[base + j], raw[base]) for j in range(1, 5)), (stride, base, kinds[base], got[base : base + 5])
    again = _episode(be, samples, counts, episode_workers.LEN_PPM, starts)
    assert np.array_equal(again.view(np.uint8), got.view(np.uint8))


@pytest.mark.parametrize("rows,stride", episode_workers.LAUNCHES)
def test_row_episode_launch_sizes(be, rows, stride):
    samples, counts, kinds = episode_workers.launch_case(rows, stride)
    _check(be, samples, counts, episode_workers.LEN_PPM, kinds, ("launch", rows, stride))
    print(f"launch {rows} x {stride}: worst so far {_worst}")


# ---- nvrx_episode_score -----------------------------------------------------------------------------------------------------
def _random_episodes(rng, R, K, S, p_missing=0.15):
    KS = K + S
    o = np.full((R, 7, KS), -1.0, dtype=np.float32)
    have = rng.random((R, KS)) >= p_missing
    excess = np.where(rng.random((R, KS)) < 0.5, 1.0, rng.uniform(1.0, 3.0, (R, KS))).astype(np.float32)
    o[:, 0, :] = np.where(have, excess, -1.0)
    for p in range(1, 7):  # (the other planes are not read: anything but the excesses)
        o[:, p, :] = np.where(have, rng.uniform(0.0, 100.0, (R, KS)), -1.0)
    return o


def _episode_score(be, episodes, T, K, S, first_rank=0, n_ranks=None):
    R = T.shape[0]
    ws = be.workspace(R, K, S, R, 0)
    ws.episode_settle()
    ws.send.copy_(torch.from_numpy(T))
    _, table, _, _ = ws.episode_buffers()
    if table.numel():
        table.copy_(torch.from_numpy(episodes.reshape(R, -1)))
    torch.cuda.synchronize()
    handle = be.episode_score(ws, table, ws.send, first_rank, n_ranks)
    got_episodes, scores = handle.records()
    lo = first_rank
    hi = R if n_ranks is None else first_rank + n_ranks
    assert np.array_equal(_bits(got_episodes), _bits(episodes[lo:hi]))  # the planes are returned unchanged
    return scores


@pytest.mark.parametrize("R,K,S", [(1, 3, 0), (8, 5, 6), (64, 17, 33), (65, 0, 64), (100, 7, 9)])
def test_episode_score_matches_numpy(be, R, K, S):
    rng = np.random.default_rng(R * 1000 + K + S)
    T = _random_table(rng, R, K, S)
    episodes = _random_episodes(rng, R, K, S)
    if R > 1 and K + S > 2:
        episodes[:, 0, 1] = rng.uniform(1.0, 2.0, R)  # a column nobody misses
    got = _episode_score(be, episodes, T, K, S)
    exp = episode_scores_table(episodes, T, K, S)
    assert got.shape == exp.shape == (R, 1 + S)
    assert np.array_equal(np.isnan(got), np.isnan(exp))
    sec_ok = ~np.isnan(exp[:, 1:])
    assert np.array_equal(_bits(got[:, 1:][sec_ok]), _bits(exp[:, 1:][sec_ok]))  # one f64 quotient rounded to f32
    gpu_ok = np.isfinite(exp[:, 0])
    if gpu_ok.any():
        assert np.abs(got[gpu_ok, 0].astype(np.float64) - exp[gpu_ok, 0].astype(np.float64)).max() <= 2e-6
    lo, n = (R // 3, max(1, R // 2)) if R > 1 else (0, 1)
    part = _episode_score(be, episodes, T, K, S, lo, n)
    assert np.array_equal(_bits(part), _bits(got[lo : lo + n]))


def test_episode_local_needs_the_ring_start_snapshot(be):
    """Without ``nvrx_onset_enable`` no report has noted where the rings start: NVRX_ERR_STATE (-1), nothing launched."""
    rings = be.make_rings(1, 4, 64)
    buf = torch.empty(7 * 4, dtype=torch.float32, device="cuda")
    try:
        rc = be.lib.nvrx_episode_local(rings.ctx, None, 5000, 0.5, buf.data_ptr(), 0, 4, 0, be.stream_handle)
        assert rc == -1 and b"snapshot" in be.lib.nvrx_last_error()
    finally:
        rings.close()


# ---- the episode step of a report ---------------------------------------------------------------------------------------------
from mp_util import run_ranks  # noqa: E402
from test_episode_host import check_headline  # noqa: E402


def _check_record(rec, x, where, len_ppm=episode_workers.LEN_PPM):
    """One record of a report against the oracle on the row ``x`` (time order): the interval is the oracle's, the rest within
    the bounds above."""
    ep = episode_one(x, len_ppm)
    ago, length, inside, outside, strength = ep.rec
    assert (rec["length"], rec["samples_ago"], rec["window"]) == (int(length), int(ago), x.size), (where, rec, ep.rec)
    assert rec["began_ago"] == (int(ago) + int(length) if length else 0)
    assert rec["open_ended"] == (bool(length) and int(ago) == ep.m), (where, rec)
    assert abs(rec["strength"] - float(strength)) <= 1.2e-7, (where, rec, strength)  # (one f32 ulp below 1)
    assert abs(rec["inside"] - float(inside)) <= float(np.spacing(inside)), (where, rec, inside)
    assert abs(rec["outside"] - float(outside)) <= float(np.spacing(outside)), (where, rec, outside)
    assert rec["excess"] == float(episode_excess(rec["length"], rec["inside"], rec["outside"], rec["strength"], 0.5)), (where, rec)


def _check_headline_gpu(s, data):
    """The headline's bounds, and every record against the oracle."""
    check_headline(s, data, exact=False)
    for i, (name, per) in enumerate(sorted(s["episodes"]["section_episodes"].items())):
        for r, rec in per.items():
            _check_record(rec, data[r, i], (name, r))


def test_headline_shape_in_one_process(be):
    data = episode_workers.headline_data()
    out = episode_workers.folded_headline(0, 1)
    assert len(out) == 3
    for entry in out:
        _check_headline_gpu(entry["report"], data)
        assert entry["report"]["tails"] == {} and entry["report"]["onsets"] == {} and entry["report"]["periods"] == {}
        assert entry["rows"] == []  # (one process: nothing is exchanged)


def test_readme_example_in_one_process(be):
    """A rank 1.5 x slower on 300 consecutive of 10 000 samples scores about 0.67 with the interval and ``samples_ago`` right,
    and stays above 0.99 on the relative, tail (0.95), onset and period scores."""
    from nvrx_straggler.folded import FoldedJob

    rng = np.random.default_rng(23)
    data = (1000.0 * (1.0 + 0.01 * rng.standard_normal((4, 2, 10000)))).astype(np.float32)
    data[2, :, 6000:6300] *= np.float32(1.5)
    job = FoldedJob(total_ranks=4, sections=2, ring_cap=10000, scores_to_compute=("relative_perf_scores",), node_name="n",
                    episode_detection=True, tail_quantile=0.95, onset_detection=True, period_detection=True)
    try:
        for lr, r in enumerate(job.logical_ranks()):
            job.load(lr, data[r])
        rep = job.report()
        t = rep.episode_scores()
        flagged = rep.identify_episode_stragglers()["straggler_sections_relative"]
        assert sorted(flagged) == sorted(t["section_scores"]) and all({s.rank for s in v} == {2} for v in flagged.values())
        for name, per in t["section_episodes"].items():
            assert (per[2]["length"], per[2]["samples_ago"], per[2]["began_ago"]) == (300, 3700, 4000), (name, per[2])
            assert abs(t["section_scores"][name][2] - 1.0 / 1.5) <= 0.02 and per[2]["strength"] > 0.95
        for other in (rep.section_relative_perf_scores, rep.tail_scores()["section_relative"], rep.onset_scores()["section_relative"],
                      rep.period_scores()["section_relative"]):
            assert all(v[2] > 0.99 for v in other.values()), other
    finally:
        job.close()


@pytest.mark.parametrize("world,others", [(2, False), (4, True)])
def test_headline_shape_on_processes_sharing_the_gpu(world, others):
    """Default route (gloo / c10d); with four processes tail, onset and period scores are on as well: four follow-up steps
    behind one report, each with its own all-gather, the episode rows last."""
    data = episode_workers.headline_data()
    res = run_ranks(episode_workers.folded_headline, world, timeout=300, use_oracle_backend=False, device=0,
                    tail_quantile=0.95 if others else 0.0, onset_detection=others, period_detection=others)
    follow_ups = 4 if others else 1
    for r in range(world):
        assert all((e["report"] is None) == (r != 0) for e in res[r])
        for i, e in enumerate(res[r]):
            # every rank: the report's own all-gather (the first report exchanges twice: once before the name sync that
            # gives its names their ids, once after), then exactly one per follow-up step, the episode rows last
            assert len(e["rows"]) == (2 if i == 0 else 1) + follow_ups and e["rows"][-1] % 7 == 0, (r, i, e["rows"])
            KS = e["rows"][-1] // 7
            if others:
                assert e["rows"][-4:] == [KS, 6 * KS, 7 * KS, 7 * KS], (r, e["rows"])
    for e in res[0]:
        rep = e["report"]
        _check_headline_gpu(rep, data)
        assert bool(rep["tails"]) == bool(rep["onsets"]) == bool(rep["periods"]) == others


@pytest.mark.parametrize("asynchronous", [False, True])
def test_next_window_written_from_another_stream_right_after_the_report(asynchronous):
    """The ordering rule: the episode kernel has read its window before the report call returns."""
    res = run_ranks(episode_workers.ring_windows_written_from_another_stream, 1, timeout=300, use_oracle_backend=False, device=0,
                    asynchronous=asynchronous)[0]
    samples, names, planted = res["samples"], res["names"], res["planted"]
    assert len(res["reports"]) == samples.shape[0] == 12
    for w, rep in enumerate(res["reports"]):
        for s, name in enumerate(names):
            rec = rep["section_episodes"][name]
            _check_record(rec, samples[w, s], (w, name))
            at, L = (int(v) for v in planted[w, s])
            # (1 % noise may move an end of the interval by a sample or two past the planted one, never far)
            assert abs(rec["length"] - L) <= 4 and abs(rec["samples_ago"] - (4096 - at - L)) <= 4 and abs(rec["excess"] - 1.5) < 0.02, (
                w, name, rec, at, L)
        # every section is slow by the same factor: one rank is its own reference
        assert all(v == 1.0 for v in rep["section_relative"].values())
        at_return, before_read, after_first, after_second = rep["copy_outs"]
        # neither the report call nor scores / stragglers copy episodes out; the first episode_scores() does, exactly once
        assert at_return == before_read == w and after_first == after_second == w + 1, (w, rep["copy_outs"])


def test_wrapped_ring_is_walked_in_time_order():
    """1.5 x ring_cap samples (and 2 x + 5) pushed into 64-deep rings, between windows that do not wrap."""
    res = run_ranks(episode_workers.wrapped_ring, 1, timeout=300, use_oracle_backend=False, device=0)[0]
    assert len(res["windows"]) == 4
    for w in res["windows"]:
        pushed = w["pushed"]
        n = min(pushed.shape[1], 64)
        for s, name in enumerate(res["names"]):
            rec = w["episodes"][name][0]
            _check_record(rec, pushed[s, -n:], name)
            assert (rec["length"], rec["samples_ago"]) == (8 + s, 10 + 3 * s) and abs(rec["excess"] - 1.5) < 0.03, (name, rec)


def test_zz_print_the_worst_figures():
    """Not a check of its own: the figures docs/MEASUREMENTS.md quotes."""
    print(f"episode kernel, all cases: {_worst}")
