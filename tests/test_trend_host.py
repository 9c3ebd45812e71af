"""Score trends, host side, on the CPU checker backend (tests/trend_oracle_backend.py): the brute-force NumPy restatement on
series worked out by hand and against a second restatement of its own, the rules that turn a record into ``falling`` /
``reports_left`` / ``identify_declining_stragglers`` at their boundaries, the option's plumbing through ReportGenerator /
Detector / Report / the Lightning callback, lifetime and pickling, that nothing is called with the option off, and the argument
checks of the two C entry points (callable without a device).

Every figure of a record is one correctly rounded operation away from the ring's entries, or a count: all comparisons are
exact."""
import copy
import ctypes
import json
import math
import pickle

import numpy as np
import pytest

import history_workers
from history_oracle_backend import fresh, history_step, stride
from trend_oracle_backend import (CountingTrendBackend, TrendOracleBackend, aged, as_dict, pair_slopes, trend_records)

NAN, INF = float("nan"), math.inf
NAN_BITS = 0x7FC00000


def _ring(column, H, S=0, slot=(1, 0)):
    """``column`` (oldest first) appended to one (family, slot) of a one-rank ring: (the ring, reports appended)."""
    f, j = slot
    hist = fresh(1, S, H)
    col = f if j == 0 else 2 + f * S + (j - 1)
    for n, x in enumerate(column):
        scores = np.full((1, 2 + 2 * S), np.nan, dtype=np.float32)
        scores[0, col] = x
        history_step(hist, scores, S, 0, 1, H, n)
    return hist, len(column)


def _trend(column, H, S=0, slot=(1, 0)):
    hist, n = _ring(column, H, S, slot)
    rec = trend_records(hist, S, H, n)
    return as_dict(rec[0, slot[0], slot[1]]), rec


def _bits(x):
    return int(np.float32(x).view(np.uint32))


# ---- 1. the restatement itself, on series worked out by hand ---------------------------------------------------------------------
def test_an_exactly_linear_fall_gives_exactly_its_slope():
    H = 16
    column = [1.0 - n / 64.0 for n in range(12)]  # -1/64 per report, every value and every pair slope exact in f32
    rec, all_rec = _trend(column, H)
    n_pairs = 12 * 11 // 2
    assert rec == {"slope": -1.0 / 64.0, "level": column[-1], "S": -n_pairs, "usable": 12}
    assert all_rec.shape == (1, 2, 1, 4) and as_dict(all_rec[0, 0, 0]) != rec  # the other family's cell holds nothing:
    assert all_rec[0, 0, 0].tolist() == [NAN_BITS, NAN_BITS, 0, 0]
    rising, _ = _trend(column[::-1], H)
    assert rising == {"slope": 1.0 / 64.0, "level": column[0], "S": n_pairs, "usable": 12}


def test_one_outlier_leaves_the_slope_within_the_clean_pair_slopes():
    rng = np.random.default_rng(5)
    clean = (0.95 - 0.012 * np.arange(16) + 0.004 * rng.standard_normal(16)).astype(np.float32)
    dirty = clean.copy()
    dirty[9] = 0.6  # one bad window
    a, _ = _trend(clean, 16)
    b, _ = _trend(dirty, 16)
    hist, n = _ring(clean, 16)
    keys, _, _ = pair_slopes(aged(hist, 0, 16, n))
    from tail_oracle_backend import key2f

    slopes = np.sort(key2f(keys[0, 1, 0]))
    lo, hi = float(slopes[len(slopes) // 4]), float(slopes[3 * len(slopes) // 4])  # the clean pair slopes' middle half
    assert lo <= b["slope"] <= hi and lo <= a["slope"] <= hi and a["slope"] < 0
    assert abs(b["slope"] - a["slope"]) < 0.002 and abs(b["level"] - a["level"]) < 0.01 and b["usable"] == 16
    # the least-squares slope of the same series moves several times as far
    t = np.arange(16, dtype=np.float64)
    ls_clean, ls_dirty = np.polyfit(t, clean.astype(np.float64), 1)[0], np.polyfit(t, dirty.astype(np.float64), 1)[0]
    assert abs(ls_dirty - ls_clean) > 3 * abs(b["slope"] - a["slope"])


def test_equal_entries_holes_and_infinities():
    rec, _ = _trend([0.625] * 9, 16)
    assert rec == {"slope": 0.0, "level": 0.625, "S": 0, "usable": 9} and math.copysign(1.0, rec["slope"]) == 1.0
    # p == 0: nothing, NaN only, infinities only -- none of them usable
    for column in ([NAN], [NAN, NAN, NAN], [INF, -INF, NAN, INF]):
        _, all_rec = _trend(column, 8)
        assert all_rec[0, 1, 0].tolist() == [NAN_BITS, NAN_BITS, 0, 0], column
    # p == 1: the slope is NaN, the level that entry, wherever it stands
    for column in ([0.8], [NAN, 0.8, NAN], [0.8, INF, NAN], [-INF, NAN, 0.8]):
        _, all_rec = _trend(column, 8)
        assert all_rec[0, 1, 0].tolist() == [NAN_BITS, _bits(0.8), 0, 1], column
    # holes and infinities between usable entries: the pair slopes divide by the AGE difference, not by the count between
    rec, _ = _trend([1.0, NAN, INF, 0.75, NAN], 8)  # ages: 0.75 at 1, 1.0 at 4
    assert rec["slope"] == float(np.float32(-0.25 / 3.0)) and rec["S"] == -1 and rec["usable"] == 2
    # v_a = x_a + slope * a: 0.75 + s and 1.0 + 4 s, in f64, rounded once; the lower median of the two
    s = float(np.float32(-0.25 / 3.0))
    assert rec["level"] == min(float(np.float32(0.75 + s)), float(np.float32(1.0 + 4 * s)))
    # 0.0 is a value; -0.0 == +0.0 for S, and the slope between them is +0.0
    rec, _ = _trend([0.0, -0.0], 4)
    assert rec["S"] == 0 and rec["usable"] == 2 and rec["slope"] == 0.0
    # the lower median of an even number of pair slopes: 3 entries, slopes {-0.25, -0.125, 0.0} -> rank 1
    rec, _ = _trend([0.75, 0.75, 0.5], 4)  # newest first: 0.5, 0.75, 0.75 -> s01 = -0.25, s02 = -0.125, s12 = 0
    assert rec["slope"] == -0.125 and rec["S"] == -2
    rec, _ = _trend([1.0, 0.5, 0.75, 0.5], 4)  # six slopes, rank (6 - 1) >> 1 = 2 of the sorted list
    x = [0.5, 0.75, 0.5, 1.0]
    slopes = sorted(float(np.float32((x[a] - x[b]) / (b - a))) for a in range(4) for b in range(a + 1, 4))
    assert rec["slope"] == slopes[2] and rec["S"] == sum((x[a] > x[b]) - (x[a] < x[b]) for a in range(4) for b in range(a + 1, 4))


def test_a_ring_that_fills_and_a_ring_that_has_wrapped():
    H = 5
    column = [1.0 - n / 32.0 for n in range(13)]
    hist = fresh(1, 0, H)
    for n, x in enumerate(column):
        history_step(hist, np.array([[np.nan, x]], dtype=np.float32), 0, 0, 1, H, n)
        rec = as_dict(trend_records(hist, 0, H, n + 1)[0, 1, 0])
        depth = min(n + 1, H)
        assert rec["usable"] == depth and rec["level"] == column[n]
        assert rec["S"] == -(depth * (depth - 1) // 2)
        assert (rec["slope"] == -1.0 / 32.0) if depth >= 2 else math.isnan(rec["slope"])
    assert stride(H) == 16 and np.isnan(hist[0, 1, 0, H:]).all()  # positions [H, stride) are never read as entries
    # the age of an entry follows the ring position: report n lives at n % H
    assert aged(hist, 0, H, 13)[0, 1, 0].tolist() == [np.float32(v) for v in column[::-1][:H]]


def _second_restatement(x):
    """The lower-median slope and S of one series (newest first), on VALUES with ``np.partition`` and plain loops."""
    ages = [a for a in range(len(x)) if np.isfinite(x[a])]
    slopes, s = [], 0
    for i, a in enumerate(ages):
        for b in ages[i + 1 :]:
            slopes.append(np.float32((float(x[a]) - float(x[b])) / float(b - a)))
            s += int(x[a] > x[b]) - int(x[a] < x[b])
    if not slopes:
        return None, s, len(ages)
    k = (len(slopes) - 1) >> 1
    return np.partition(np.array(slopes, dtype=np.float32), k)[k], s, len(ages)


def test_the_restatement_agrees_with_a_second_one_of_its_own():
    rng = np.random.default_rng(11)
    H, S, n_ranks = 17, 3, 4
    hist = fresh(n_ranks, S, H)
    steps = 2 * H + 3
    for n in range(steps):
        scores = (0.8 + 0.05 * rng.standard_normal((n_ranks, 2 + 2 * S))).astype(np.float32)
        scores[rng.random(scores.shape) < 0.15] = np.nan
        scores[rng.random(scores.shape) < 0.03] = np.inf
        scores[:, 3] = np.round(scores[:, 3] * 16) / 16  # a column on a coarse grid: tied slopes
        history_step(hist, scores, S, 0, n_ranks, H, n)
        if n % 7 and n != steps - 1:
            continue
        rec = trend_records(hist, S, H, n + 1)
        x = aged(hist, S, H, n + 1)
        for r in range(n_ranks):
            for f in range(2):
                for j in range(1 + S):
                    slope, s, p = _second_restatement(x[r, f, j])
                    got = as_dict(rec[r, f, j])
                    assert got["S"] == s and got["usable"] == p
                    if slope is None:
                        assert math.isnan(got["slope"])
                    else:
                        assert got["slope"] == float(slope), (n, r, f, j)  # (no signed zeros among these slopes' ties)
                        v = sorted(float(np.float32(float(x[r, f, j, a]) + float(slope) * a)) for a in range(x.shape[-1])
                                   if np.isfinite(x[r, f, j, a]))
                        assert got["level"] == v[(p - 1) >> 1]


# ---- 2. from a record to falling / reports_left / declining ----------------------------------------------------------------------
class _Handle:
    def __init__(self, rec):
        self.rec, self.reads = rec, 0

    def records(self):
        self.reads += 1
        return self.rec


def _report_with(records, min_reports=6, min_tau=0.6, horizon=8, thresholds=(0.75, 0.7, 0.8, 0.75), sections=None):
    """A Report whose trends are ``records`` ([n_ranks, 2, 1 + S, 4] words given as (slope, level, S, usable) tuples)."""
    import callback_script
    from nvrx_straggler.reporting import Report, _TrendSource

    rec = np.zeros(np.shape(records)[:-1] + (4,), dtype=np.uint32)
    arr = np.asarray(records, dtype=np.float64)
    rec[..., 0] = arr[..., 0].astype(np.float32).view(np.uint32)
    rec[..., 1] = arr[..., 1].astype(np.float32).view(np.uint32)
    rec[..., 2] = arr[..., 2].astype(np.int32).view(np.uint32)
    rec[..., 3] = arr[..., 3].astype(np.uint32)
    n = rec.shape[0]
    fields = dict(callback_script.reports(n)[1])
    rep = Report(**fields)
    handle = _Handle(rec)
    rep.__dict__["_trends"] = _TrendSource(handle, range(n), sections or {}, True, True, 8, min_reports, min_tau, horizon,
                                           thresholds)
    return rep, handle


def test_the_rules_at_their_boundaries():
    thr = 0.75
    cells = [
        # (slope, level, S, usable)                          falling  reports_left
        ((-0.0125, 0.8, -15, 6), True, 4),                   # tau = -1; (0.8 - 0.75) / 0.0125 = 4 (in f32 values: see below)
        ((-0.0125, 0.8, -9, 6), True, 4),                    # tau = -9 / 15 = -0.6 == -min_tau exactly: falling
        ((-0.0125, 0.8, -8, 6), False, None),                # tau = -0.533: not
        ((-0.0125, 0.8, -10, 5), False, None),               # usable == min_reports - 1 (tau = -1): not
        ((-0.0, 0.8, -15, 6), False, None),                  # slope == -0.0 is not < 0
        ((0.0125, 0.8, 15, 6), False, None),                 # rising
        ((-0.0125, 0.75, -15, 6), True, 0),                  # level == thr: not below, and (level - thr) / -slope = 0
        ((-0.0125, 0.7499999, -15, 6), True, 0),             # level < thr
        ((0.0125, 0.7, 15, 6), False, 0),                    # below already, whatever the trend: 0, and not falling
        ((NAN, 0.7, 0, 1), False, 0),
        ((NAN, NAN, 0, 0), False, None),
        ((-0.001, 0.9, -15, 6), True, None),                 # (filled in below: a long way off)
    ]
    records = np.array([[[c[0]], [c[0]]] for c in cells], dtype=np.float64)  # [ranks, 2, 1, 4]: both families the same
    rep, handle = _report_with(records, thresholds=(thr, thr, thr, thr))
    assert handle.reads == 0
    t = rep.score_trends()
    assert handle.reads == 1 and rep.score_trends() == t and handle.reads == 1
    json.dumps(t)
    assert {k: t[k] for k in ("depth", "min_reports", "min_tau", "horizon", "thresholds")} == {
        "depth": 8, "min_reports": 6, "min_tau": 0.6, "horizon": 8, "thresholds": (thr,) * 4}
    assert t["section_relative"] == {} == t["section_individual"]
    for r, (cell, falling, left) in enumerate(cells):
        rec = t["gpu_relative"][r]
        assert json.dumps(rec) == json.dumps(t["gpu_individual"][r])
        slope32, level32 = float(np.float32(cell[0])), float(np.float32(cell[1]))
        assert rec["usable"] == cell[3] and rec["falling"] is falling, (r, rec)
        assert rec["tau"] == (cell[2] / (cell[3] * (cell[3] - 1) // 2) if cell[3] >= 2 else 0.0)
        if r == len(cells) - 1:
            left = math.ceil((level32 - thr) / -slope32)
            assert left in (150, 151)
        if r in (0, 1):
            left = math.ceil((level32 - thr) / -slope32)  # the f32 level 0.8 is a hair above 0.8: 5, not 4
            assert left in (4, 5)
        assert rec["reports_left"] == left, (r, rec)
        assert (math.isnan(rec["slope"]) and math.isnan(cell[0])) or rec["slope"] == slope32
    ranks = history_workers.ranks_of
    declining = rep.identify_declining_stragglers()
    assert sorted(declining) == ["straggler_gpus_individual", "straggler_gpus_relative", "straggler_sections_individual",
                                 "straggler_sections_relative"]
    assert sorted(s.rank for s in declining["straggler_gpus_relative"]) == [0, 1, 6, 7]  # falling and within 8 reports
    assert sorted(s.rank for s in rep.identify_declining_stragglers(0)["straggler_gpus_relative"]) == [6, 7]
    assert sorted(s.rank for s in rep.identify_declining_stragglers(1000)["straggler_gpus_individual"]) == [0, 1, 6, 7, 11]
    left0 = t["gpu_relative"][0]["reports_left"]
    assert ranks(rep.identify_declining_stragglers(left0 - 1)) == [6, 7] and 0 in ranks(rep.identify_declining_stragglers(left0))
    for bad in (-1, 2.5, "3", True):
        with pytest.raises(ValueError, match="horizon must be an integer >= 0"):
            rep.identify_declining_stragglers(bad)
    # the thresholds are per family and slot: (gpu_rel, section_rel, gpu_indiv, section_indiv)
    records = np.array([[[(-0.01, 0.78, -15, 6)] * 2] * 2], dtype=np.float64)  # one rank, both families, GPU slot + one section
    rep, _ = _report_with(records, thresholds=(0.75, 0.7, 0.8, 0.5), sections={"fwd": 0})
    t = rep.score_trends()
    level = float(np.float32(0.78))
    slope = float(np.float32(-0.01))
    assert t["gpu_relative"][0]["reports_left"] == math.ceil((level - 0.75) / -slope)
    assert t["section_relative"]["fwd"][0]["reports_left"] == math.ceil((level - 0.7) / -slope)
    assert t["gpu_individual"][0]["reports_left"] == 0  # 0.78 < 0.8
    assert t["section_individual"]["fwd"][0]["reports_left"] == math.ceil((level - 0.5) / -slope) == 28
    found = rep.identify_declining_stragglers()
    assert ranks({"a": found["straggler_gpus_relative"]}) == [0] and "fwd" in found["straggler_sections_relative"]
    assert "fwd" not in found["straggler_sections_individual"]  # 28 reports off, beyond the horizon of 8
    # a private copy each time
    t["gpu_relative"].clear()
    assert rep.score_trends()["gpu_relative"]


# ---- 3. the option's values -------------------------------------------------------------------------------------------------
@pytest.fixture
def cpu_backend():
    from nvrx_straggler import backend

    be = TrendOracleBackend()
    backend.set_backend(be)
    try:
        yield be
    finally:
        backend.set_backend(None)


def test_option_values(cpu_backend, monkeypatch):
    from nvrx_straggler import Detector
    from nvrx_straggler.reporting import ReportGenerator

    for depth in (0, 2, 3):
        with pytest.raises(ValueError, match=r"score_trends needs a score history of at least 4 reports"):
            ReportGenerator(["relative_perf_scores"], score_history=depth, persistence_min_reports=min(depth, 3) or 3,
                            score_trends=True)
    for bad in (3, 9, 0, -1, 6.0, "6", None, True):
        with pytest.raises(ValueError, match=r"trend_min_reports must be an integer within \[4, score_history=8\]"):
            ReportGenerator(["relative_perf_scores"], score_history=8, score_trends=True, trend_min_reports=bad)
    for bad in (0, 0.0, -0.5, 1.0001, NAN, INF, "x", None, True):
        with pytest.raises(ValueError, match=r"trend_min_tau must be a number within \(0, 1\]"):
            ReportGenerator(["relative_perf_scores"], score_history=8, score_trends=True, trend_min_tau=bad)
    for bad in (-1, 2.5, "8", True):
        with pytest.raises(ValueError, match=r"trend_horizon must be None \(the history's depth\) or an integer >= 0"):
            ReportGenerator(["relative_perf_scores"], score_history=8, score_trends=True, trend_horizon=bad)
    gen = ReportGenerator(["relative_perf_scores"], score_history=16, score_trends=True)
    assert (gen.score_trends, gen.trend_min_reports, gen.trend_min_tau, gen.trend_horizon) == (True, 6, 0.6, 16)
    gen = ReportGenerator(["relative_perf_scores"], score_history=4, score_trends=True, trend_min_reports=4, trend_min_tau=1,
                          trend_horizon=0)
    assert (gen.trend_min_reports, gen.trend_min_tau, gen.trend_horizon) == (4, 1.0, 0)
    off = ReportGenerator(["relative_perf_scores"], trend_min_reports=99, trend_min_tau=7, trend_horizon=-3)  # (ignored while off)
    assert off.score_trends is False
    off = ReportGenerator(["relative_perf_scores"], score_history=8)
    assert off.score_trends is False and off._history is not None
    # the environment variable is the Detector's default, read only when the argument is None
    monkeypatch.setenv("NVRX_SCORE_HISTORY", "16")
    monkeypatch.setenv("NVRX_SCORE_TRENDS", "1")
    Detector.initialize(node_name="n0")
    try:
        r = Detector.reporter
        assert (r.score_history, r.score_trends, r.trend_min_reports, r.trend_min_tau, r.trend_horizon) == (16, True, 6, 0.6, 16)
    finally:
        Detector.shutdown()
    Detector.initialize(node_name="n0", score_trends=False)
    try:
        assert Detector.reporter.score_trends is False and Detector.reporter.score_history == 16
    finally:
        Detector.shutdown()
    monkeypatch.setenv("NVRX_SCORE_TRENDS", "0")
    Detector.initialize(node_name="n0")
    try:
        assert Detector.reporter.score_trends is False
    finally:
        Detector.shutdown()
    monkeypatch.delenv("NVRX_SCORE_TRENDS")
    monkeypatch.delenv("NVRX_SCORE_HISTORY")
    Detector.initialize(node_name="n0", score_history=4, persistence_min_reports=2, score_trends=True, trend_min_tau=0.8,
                        trend_horizon=3)
    try:
        r = Detector.reporter
        assert (r.score_trends, r.trend_min_reports, r.trend_min_tau, r.trend_horizon) == (True, 4, 0.8, 3)  # (6, capped)
    finally:
        Detector.shutdown()
    with pytest.raises(ValueError, match="score_trends needs a score history"):
        Detector.initialize(node_name="n0", score_trends=True)
    assert not Detector.initialized
    Detector.initialize(node_name="n0")
    try:
        assert Detector.reporter.score_trends is False and Detector.reporter.score_history == 0
    finally:
        Detector.shutdown()


def test_option_needs_a_backend_with_score_trends():
    from history_oracle_backend import HistoryOracleBackend
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator

    backend.set_backend(HistoryOracleBackend())
    try:
        with pytest.raises(RuntimeError, match="no score trends"):
            ReportGenerator(["relative_perf_scores"], score_history=8, score_trends=True)
        ReportGenerator(["relative_perf_scores"], score_history=8)
    finally:
        backend.set_backend(None)


# ---- 4. off by default: nothing is called -----------------------------------------------------------------------------------
@pytest.mark.parametrize("emulate_fused,asynchronous", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("history", [0, 8])
def test_default_is_off_and_calls_nothing(emulate_fused, asynchronous, history):
    from nvrx_straggler import Statistic as S
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator

    be = CountingTrendBackend(emulate_fused=emulate_fused)
    backend.set_backend(be)
    try:
        gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=True, node_name="n",
                              asynchronous=asynchronous, score_history=history)
        summ = {S.MIN: 1.0, S.MAX: 2.0, S.MED: 1.5, S.AVG: 1.5, S.STD: 0.1, S.NUM: 4}
        rep = gen.generate_report({"sec": summ}, {"k": summ})
        nobody = {"straggler_gpus_relative": set(), "straggler_gpus_individual": set(), "straggler_sections_relative": {},
                  "straggler_sections_individual": {}}
        assert rep.score_trends() == {} and pickle.loads(pickle.dumps(rep)).score_trends() == {}
        assert rep.identify_declining_stragglers() == nobody and rep.identify_declining_stragglers(5) == nobody
        rings = be.make_rings(1, 8, 16)
        rows = {"sec": rings.row_for(0, "sec")}
        for i in range(3):
            rings.push_many(rows["sec"], [5.0 + i, 6.0])
            rep = gen.generate_report_from_rings(rings, rows, {})
            rings.reset()
            assert rep.score_trends() == {} and "_trends" not in rep.__dict__
        assert gen._ring_plan is not None and be.trend_calls == 0 and be.history_calls == (4 if history else 0)
        gen.close()
    finally:
        backend.set_backend(None)


# ---- 5. the headline scenario: a rank that loses a percent per report ---------------------------------------------------------
RANKS, REPORTS, FALLS_RANK, FALLS_FROM, ONCE_RANK, ONCE_REPORT = 8, 44, 5, 8, 2, 14


def _window(report, samples=9):
    """``[RANKS, 2, samples]`` f32: 8 ranks around 1000 with 1 % noise; rank 5 gets 1.2 % slower per report from report 8 on,
    rank 2 is 1.4 x slower in report 14 only."""
    rng = np.random.default_rng([23, report])
    x = 1000.0 * (1.0 + 0.01 * rng.standard_normal((RANKS, 2, samples)))
    x[FALLS_RANK] *= 1.0 + 0.012 * max(0, report - FALLS_FROM)
    if report == ONCE_REPORT:
        x[ONCE_RANK] *= 1.4
    return x.astype(np.float32)


def _scenario(be, **options):
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=True, node_name="n", **options)
    rings = be.make_rings(RANKS, 2, 16)
    rows = {n: rings.row_for(0, n) for n in ("fwd", "bwd")}
    out = []
    try:
        for i in range(REPORTS):
            w = _window(i)
            for lr in range(RANKS):
                for s, n in enumerate(rows):
                    rings.push_many(rows[n], w[lr, s], lr=lr)
            out.append(gen.generate_report_from_rings(rings, rows, {}, local_ranks=RANKS))
            rings.reset()
    finally:
        gen.close()
    return out


@pytest.mark.parametrize("emulate_fused", [False, True])
def test_a_falling_rank_is_named_before_any_other_rule_and_a_single_bad_window_never(emulate_fused):
    from nvrx_straggler import backend

    be = TrendOracleBackend(emulate_fused=emulate_fused)
    backend.set_backend(be)
    try:
        reports = _scenario(be, score_history=16, persistence_min_reports=3, score_trends=True)
    finally:
        backend.set_backend(None)
    ranks = history_workers.ranks_of
    assert be.trend_calls == REPORTS == be.history_calls and all(h.reads == 0 for h in be.trend_handles)
    assert [a[2] for a in be.trend_args] == list(range(1, REPORTS + 1))  # n_reports: the history step's report included
    assert all(a[:2] == ((0, RANKS), 2) for a in be.trend_args)
    first = {}
    for i, rep in enumerate(reports):
        for rule, found in (("declining", rep.identify_declining_stragglers()), ("single", rep.identify_stragglers()),
                            ("persistent", rep.identify_persistent_stragglers())):
            named = ranks(found)
            if rule == "declining":
                assert ONCE_RANK not in named, (i, found)  # one bad window is never a trend
                assert set(named) <= {FALLS_RANK}, (i, found)
            if FALLS_RANK in named:
                first.setdefault(rule, i)
        t = rep.score_trends()
        json.dumps(t)
        assert t["depth"] == min(i + 1, 16) and t["min_reports"] == 6 and t["min_tau"] == 0.6 and t["horizon"] == 16
        assert t["thresholds"] == (0.75,) * 4 and "gpu_individual" not in t and "section_individual" not in t
        assert sorted(t["section_relative"]) == ["bwd", "fwd"] and sorted(t["gpu_relative"]) == list(range(RANKS))
        assert all(rec["usable"] == 0 and rec["reports_left"] is None for rec in t["gpu_relative"].values())  # (no kernels)
        for name in ("fwd", "bwd"):
            for r, rec in t["section_relative"][name].items():
                assert rec["usable"] == t["depth"] and -1.0 <= rec["tau"] <= 1.0
    # named by the trend several reports before its score first crosses 0.75, and before it has stayed there for three
    assert first["declining"] + 4 <= first["single"] < first["persistent"], first
    i = first["declining"]
    rec = reports[i].score_trends()["section_relative"]
    left = min(rec[n][FALLS_RANK]["reports_left"] for n in rec if rec[n][FALLS_RANK]["falling"])
    assert abs((i + left) - first["single"]) <= 4, (first, left)  # ... and the forecast is about right
    # the records are the restatement's on the reports' own scores
    hist = fresh(RANKS, 64, 16)
    for i, rep in enumerate(reports):
        scores = np.full((RANKS, 2 + 2 * 2), np.nan, dtype=np.float32)
        for s, name in enumerate(("fwd", "bwd")):
            scores[:, 2 + 2 + s] = [rep.section_relative_perf_scores[name][r] for r in range(RANKS)]
        history_step(hist, scores, 2, 0, RANKS, 16, i)
        want = trend_records(hist, 2, 16, i + 1)
        t = rep.score_trends()
        for s, name in enumerate(("fwd", "bwd")):
            for r in range(RANKS):
                w, g = as_dict(want[r, 1, 1 + s]), t["section_relative"][name][r]
                assert (g["slope"], g["level"], g["usable"]) == (w["slope"], w["level"], w["usable"]) or i == 0
                pairs = w["usable"] * (w["usable"] - 1) // 2
                assert g["tau"] == (w["S"] / pairs if pairs else 0.0)


# ---- 6. lifetime and pickling -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("emulate_fused,asynchronous", [(False, False), (True, False), (True, True)])
def test_a_held_report_keeps_its_trends_and_reports_travel(emulate_fused, asynchronous):
    from nvrx_straggler import Statistic as S
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator

    be = TrendOracleBackend(emulate_fused=emulate_fused)
    backend.set_backend(be)
    try:
        gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=True, node_name="n",
                              score_history=8, persistence_min_reports=2, score_trends=True, trend_min_reports=4,
                              asynchronous=asynchronous)
        rings = be.make_rings(1, 8, 16)
        kernel_rows, section_rows = {"gemm": rings.row_for(1, "gemm")}, {"sec": rings.row_for(0, "sec")}
        held = []
        for w in range(6):
            v = np.arange(1, 12, dtype=np.float32) * (w + 1)  # every window slower: the individual scores fall 1, 1/2, 1/3 ...
            rings.push_many(kernel_rows["gemm"], v)
            rings.push_many(section_rows["sec"], v + 0.5)
            held.append(gen.generate_report_from_rings(rings, section_rows, kernel_rows))
            rings.reset()
        assert be.trend_calls == 6 and all(h.reads == 0 for h in be.trend_handles)
        for w in (2, 5, 4, 3, 0, 1):  # a report read after the next two were issued is still its own
            t = held[w].score_trends()
            assert be.trend_handles[w].reads == 1
            assert t["depth"] == w + 1 and t["gpu_relative"][0]["usable"] == w + 1
            assert (t["gpu_relative"][0]["slope"] == 0.0) == (w >= 1) and t["gpu_relative"][0]["tau"] == 0.0  # 1.0 throughout
            gi = t["gpu_individual"][0]
            assert gi["usable"] == w + 1 and gi["tau"] == (-1.0 if w else 0.0) and (math.isnan(gi["slope"]) if w == 0 else gi["slope"] < 0)
            assert gi["falling"] == (w + 1 >= 4)
            assert gi["reports_left"] == (0 if gi["level"] < 0.75 else None if not gi["falling"] else gi["reports_left"])
            assert history_workers.ranks_of(held[w].identify_declining_stragglers()) == ([0] if w + 1 >= 4 else [])
            assert held[w].score_trends() == t and be.trend_handles[w].reads == 1
            for clone in (pickle.loads(pickle.dumps(held[w])), copy.deepcopy(held[w])):
                assert json.dumps(clone.score_trends()) == json.dumps(t)
                assert clone.identify_declining_stragglers() == held[w].identify_declining_stragglers()
                assert json.dumps(clone.score_history()) == json.dumps(held[w].score_history())
        # the dict-input path goes through the same score kernel: history and trends follow it too
        summ = {S.MIN: 1.0, S.MAX: 2.0, S.MED: 1.5, S.AVG: 1.5, S.STD: 0.1, S.NUM: 4}
        t = gen.generate_report({"sec": summ}, {"gemm": summ}).score_trends()
        assert t["depth"] == 7 and t["section_relative"]["sec"][0]["usable"] == 7 and be.trend_calls == 7
        # a restart of the history restarts the trends
        gen.reset_score_history()
        t = gen.generate_report({"sec": summ}, {"gemm": summ}).score_trends()
        assert t["depth"] == 1 and t["gpu_relative"][0]["usable"] == 1 and math.isnan(t["gpu_relative"][0]["slope"])
        gen.close()
    finally:
        backend.set_backend(None)


def test_a_pickled_report_carries_its_trends_materialised():
    records = np.array([[[(-0.0125, 0.8, -15, 6)], [(0.01, 0.9, 15, 6)]]], dtype=np.float64)
    rep, handle = _report_with(records)
    clone = pickle.loads(pickle.dumps(rep))
    assert handle.reads == 1 and isinstance(clone.__dict__["_trends"], dict)
    assert clone.score_trends() == rep.score_trends() and clone.score_trends()["gpu_individual"][0]["falling"] is True
    assert clone.score_history() == {} == rep.score_history()


# ---- 7. the Lightning callback ------------------------------------------------------------------------------------------------
def _scripted_trends(declining):
    def rec(left):
        if left is None:
            return {"slope": 0.001, "level": 0.93, "tau": 0.1, "usable": 8, "falling": False, "reports_left": None}
        return {"slope": -0.0125, "level": 0.75 + 0.0125 * left, "tau": -0.9, "usable": 8, "falling": True, "reports_left": left}

    return {"depth": 8, "min_reports": 6, "min_tau": 0.6, "horizon": 8, "thresholds": (0.7, 0.75, 0.7, 0.75),
            "gpu_relative": {r: rec(declining.get(r)) for r in range(8)}, "gpu_individual": {r: rec(None) for r in range(8)},
            "section_relative": {}, "section_individual": {}}


def test_callback_warns_of_a_declining_rank_and_never_halts_for_it(monkeypatch):
    import callback_script
    import nvrx_straggler
    from nvidia_resiliency_ext.ptl_resiliency import StragglerDetectionCallback
    from nvrx_straggler.reporting import Report

    healthy = callback_script._scores(8)
    base = {k: v for k, v in callback_script.reports(8)[1].items() if not k.startswith("gpu_")}
    sequence = [{}, {5: 7}, None, {5: 3, 2: 8}, {}, {5: 12}]  # (rank -> reports_left); 12 is beyond the horizon of 8

    def scripted(n_ranks):
        return [None if e is None else dict(base, gpu_relative_perf_scores=healthy, gpu_individual_perf_scores=healthy,
                                            trends=_scripted_trends(e)) for e in sequence]

    def make_report(trends=None, **fields):
        rep = Report(**fields)
        rep.__dict__["_trends"] = trends
        return rep

    monkeypatch.setattr(callback_script, "reports", scripted)
    monkeypatch.setitem(callback_script.CONFIGS, "declining", dict(callback_script.CONFIGS["print2_log_stop"], warn_if_declining=True))
    got = callback_script.drive(StragglerDetectionCallback, nvrx_straggler, make_report,
                                ("declining", "declining", 8, 0, False, False, False))
    assert got["initialize_calls"] == [dict(scores_to_compute=["relative_perf_scores", "individual_perf_scores"],
                                            gather_on_rank0=True, profiling_interval=1, report_time_interval=1.0, score_history=8,
                                            persistence_thresholds=[0.7, 0.75, 0.7, 0.75], score_trends=True)]
    its = got["iterations"]
    warnings = [[m for level, m in it["records"] if level == "WARNING"] for it in its]
    assert [len(w) for w in warnings] == [0, 1, 0, 1, 0, 0]  # one warning per report that names anybody
    assert warnings[1] == ["STRAGGLER DETECTION WARNING: Some GPUs are getting slower: rank 5 relative GPU score falls 0.0125 "
                           "per report (level 0.838, reports_left=7)"]
    assert "rank 2 relative" in warnings[3][0] and "reports_left=8" in warnings[3][0] and "rank 5" in warnings[3][0]
    assert "reports_left=3" in warnings[3][0]
    assert [it["should_stop"] for it in its] == [False] * len(sequence) and all(it["exit"] is None for it in its)  # stop_if_detected=True
    # together with min_consecutive_reports: one history serves both
    monkeypatch.setitem(callback_script.CONFIGS, "both", dict(callback_script.CONFIGS["print2_log_stop"], warn_if_declining=True,
                                                              min_consecutive_reports=12))
    cb = StragglerDetectionCallback(**callback_script.CONFIGS["both"])
    assert cb.warn_if_declining is True and cb.min_consecutive_reports == 12

    # the default, given or not: the initialize call and the transcript of today
    monkeypatch.undo()
    monkeypatch.setitem(callback_script.CONFIGS, "explicit_off", dict(callback_script.CONFIGS["print2_log_stop"], warn_if_declining=False))
    plain = callback_script.drive(StragglerDetectionCallback, nvrx_straggler, Report, callback_script.SCENARIOS[0])
    given = callback_script.drive(StragglerDetectionCallback, nvrx_straggler, Report,
                                  ("rank0_8ranks", "explicit_off", 8, 0, False, False, False))
    assert json.dumps(dict(given, config=None), sort_keys=True) == json.dumps(dict(plain, config=None), sort_keys=True)
    assert given["initialize_calls"] == [dict(scores_to_compute=["relative_perf_scores", "individual_perf_scores"],
                                              gather_on_rank0=True, profiling_interval=1, report_time_interval=1.0)]


def test_callback_with_both_switches_asks_for_one_history(monkeypatch):
    import callback_script
    import nvrx_straggler
    from nvidia_resiliency_ext.ptl_resiliency import StragglerDetectionCallback
    from nvrx_straggler.reporting import Report

    monkeypatch.setitem(callback_script.CONFIGS, "both", dict(callback_script.CONFIGS["quiet_rel_only"], warn_if_declining=True,
                                                              min_consecutive_reports=12))
    got = callback_script.drive(StragglerDetectionCallback, nvrx_straggler, Report, ("both", "both", 8, 1, False, False, False))
    assert got["initialize_calls"] == [dict(scores_to_compute=["relative_perf_scores"], gather_on_rank0=True, profiling_interval=3,
                                            report_time_interval=5.0, score_history=12, persistence_min_reports=12,
                                            persistence_thresholds=[0.9, 0.75, 0.5, 0.75], score_trends=True)]


# ---- 8. header, bindings and macros agree; the C entry points check their arguments before any device is touched ----------------
def test_entry_points_check_their_arguments_without_a_device():
    import os
    import re

    from nvrx_straggler import _native

    lib = _native.load()
    assert {"nvrx_score_trend", "nvrx_report_trend"} <= {name for name, _, _ in _native.SYMBOLS}
    assert lib.nvrx_abi_version() == 2
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nvrx_straggler.h")).read()
    assert re.search(r"#define NVRX_ABI_VERSION 2\b", header)
    assert "#define NVRX_TREND_WORDS(n_ranks, S) ((size_t)(n_ranks) * 2 * (1 + (size_t)(S)) * 4)" in header
    assert _native.TREND_RECORD_WORDS == 4 and _native.trend_words(8, 64) == 8 * 2 * 65 * 4
    flat = " ".join(header.split())
    assert ("int nvrx_score_trend(const float *d_hist, int n_ranks, int S, int S_cap, int H, uint64_t n_reports, void *d_out, "
            "void *stream);") in flat
    assert ("int nvrx_report_trend(nvrx_ctx *ctx, const float *d_hist, int n_ranks, int S, int S_cap, int H, uint64_t n_reports, "
            "void *d_out);") in flat
    by_name = {name: (res, args) for name, res, args in _native.SYMBOLS}
    c = ctypes
    assert by_name["nvrx_score_trend"] == (c.c_int, [c.c_void_p, c.c_int, c.c_int, c.c_int, c.c_int, c.c_uint64, c.c_void_p,
                                                     c.c_void_p])
    assert by_name["nvrx_report_trend"] == (c.c_int, [c.c_void_p, c.c_void_p, c.c_int, c.c_int, c.c_int, c.c_int, c.c_uint64,
                                                      c.c_void_p])
    fake = ctypes.c_void_p(4096)

    def step(hist=fake, n=8, S=2, cap=64, H=8, reports=3, out=fake):
        return lib.nvrx_score_trend(hist, n, S, cap, H, reports, out, None)

    for H in (1, 0, -4, 65, 1000):
        assert step(H=H) == _native.ERR_RANGE and b"depth" in lib.nvrx_last_error()
    assert step(n=0) == _native.ERR_INVALID and step(n=-1) == _native.ERR_INVALID and step(S=-1) == _native.ERR_INVALID
    assert b"shape" in lib.nvrx_last_error()
    assert step(S=65) == _native.ERR_INVALID and b"S_cap" in lib.nvrx_last_error()
    assert step(cap=1 << 20, S=1 << 20) == _native.ERR_RANGE
    assert step(reports=0) == _native.ERR_INVALID and b"n_reports" in lib.nvrx_last_error()
    assert step(hist=None) == _native.ERR_INVALID and step(out=None) == _native.ERR_INVALID and b"null" in lib.nvrx_last_error()
    assert step(hist=ctypes.c_void_p(4100)) == _native.ERR_INVALID and b"aligned" in lib.nvrx_last_error()
    assert step(out=ctypes.c_void_p(4104)) == _native.ERR_INVALID

    def report(ctx=fake, hist=fake, n=8, S=2, cap=64, H=8, reports=3, out=fake):
        return lib.nvrx_report_trend(ctx, hist, n, S, cap, H, reports, out)

    assert report(ctx=None) == _native.ERR_INVALID
    assert report(H=1) == _native.ERR_RANGE and report(H=65) == _native.ERR_RANGE
    assert report(n=0) == _native.ERR_INVALID and report(S=3, cap=2) == _native.ERR_INVALID and report(reports=0) == _native.ERR_INVALID
    assert report(hist=None) == _native.ERR_INVALID and report(out=ctypes.c_void_p(4104)) == _native.ERR_INVALID
