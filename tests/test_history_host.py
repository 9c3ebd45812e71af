"""The score history, host side, on the CPU checker backend (tests/history_oracle_backend.py): the NumPy restatement on rows
worked out by hand, the option's plumbing through ReportGenerator / Detector / Report / the Lightning callback, the headline
scenario (one slow window flags nobody, a rank that stays slow is flagged at its third report), new sections, growth,
restart, lifetime and pickling, that the option adds no collective on gloo ranks and changes nothing else a report says, and
the argument checks of the two C entry points (callable without a device).

Every figure of a record is an actual score or a count: all comparisons are exact."""
import copy
import ctypes
import json
import math
import pickle

import numpy as np
import pytest

import history_workers
from history_oracle_backend import (CountingHistoryBackend, HistoryOracleBackend, as_dicts, fresh, history_step, stride,
                                    threshold_table)
from mp_util import run_ranks

NAN = float("nan")


@pytest.fixture
def cpu_backend():
    from nvrx_straggler import backend

    be = HistoryOracleBackend()
    backend.set_backend(be)
    try:
        yield be
    finally:
        backend.set_backend(None)


def _feed(column, H, thresholds=None, S=0, slot=(1, 0)):
    """Append ``column`` (oldest first) to one (family, slot) of a one-rank ring; the last step's record, as a dict."""
    f, j = slot
    hist = fresh(1, S, H)
    col = f if j == 0 else 2 + f * S + (j - 1)
    rec = None
    for n, x in enumerate(column):
        scores = np.full((1, 2 + 2 * S), np.nan, dtype=np.float32)
        scores[0, col] = x
        rec = history_step(hist, scores, S, 0, 1, H, n, thresholds)[0, f, j]
    return as_dicts(rec), int(rec[7]), hist


# ---- 1. the restatement itself, on rows worked out by hand -----------------------------------------------------------------------
def test_restatement_on_hand_written_rows():
    newest_first = [0.7, NAN, 0.6, 0.8, math.inf, 0.0]
    rec, depth, hist = _feed(newest_first[::-1], H=8)
    assert depth == 6 and rec["latest"] == np.float32(0.7)
    assert (rec["streak"], rec["below"], rec["present"]) == (1, 3, 5)  # the NaN ends the streak; +inf and 0.0 are values
    assert rec["median"] == np.float32(0.7) and rec["worst"] == 0.0 and rec["best"] == math.inf  # sorted: 0 .6 .7 .8 inf
    assert stride(8) == 16 and hist.shape == (1, 2, 1, 16)
    assert np.isnan(hist[0, 1, 0, 6:]).all() and np.isnan(hist[0, 0]).all()  # nothing else was touched
    # a score equal to the threshold is not below; the comparison is the flags': (double)x < thr
    rec, _, _ = _feed([0.5, 0.75, 0.5], H=4)
    assert (rec["streak"], rec["below"], rec["present"]) == (1, 2, 3) and rec["median"] == 0.5
    rec, _, _ = _feed([0.5, 0.75, 0.5], H=4, thresholds=(0.7500001, 0.75, 0.75, 0.75))
    assert (rec["streak"], rec["below"]) == (3, 3)
    rec, _, _ = _feed([0.5, 0.5], H=4, thresholds=(0.9, 0.9, 0.5, 0.5), slot=(0, 0))  # the individual GPU score: thresholds[2]
    assert (rec["streak"], rec["below"]) == (0, 0)
    # the ring wraps: depth stops at H, the oldest entries leave, the streak ends with the depth
    rec, depth, hist = _feed([0.9, 0.1, 0.2, 0.3, 0.4], H=3)
    assert depth == 3 and (rec["streak"], rec["below"], rec["present"]) == (3, 3, 3)
    assert (rec["worst"], rec["median"], rec["best"]) == (np.float32(0.2), np.float32(0.3), np.float32(0.4))
    assert hist[0, 1, 0, :3].tolist() == [np.float32(0.3), np.float32(0.4), np.float32(0.2)]  # report n lives at n % H
    # nothing present: the order statistics are NaN, the counts zero
    rec, _, _ = _feed([NAN, NAN], H=2)
    assert rec["present"] == 0 and rec["streak"] == 0 and all(math.isnan(rec[k]) for k in ("latest", "median", "worst", "best"))
    # the lower median of an even count; ties; -0.0 orders before +0.0
    rec, _, _ = _feed([0.4, 0.4, 0.9, 0.9], H=16)
    assert rec["median"] == np.float32(0.4)
    rec, _, _ = _feed([0.0, -0.0], H=2)
    assert math.copysign(1.0, rec["worst"]) == -1.0 and math.copysign(1.0, rec["best"]) == 1.0
    # sections read their own columns and thresholds; slots above S are left alone
    t = threshold_table(2, (0.1, 0.2, 0.3, 0.4))
    assert t.tolist() == [[0.3, 0.4, 0.4], [0.1, 0.2, 0.2]]
    hist = fresh(2, 3, 2)
    scores = np.arange(3 * 6, dtype=np.float32).reshape(3, 6) / 100
    rec = history_step(hist, scores, 2, 1, 2, 2, 0)
    assert rec.shape == (2, 2, 3, 8) and np.isnan(hist[:, :, 3]).all()
    assert hist[1, 0, :3, 0].tolist() == scores[2, [0, 2, 3]].tolist() and hist[0, 1, :3, 0].tolist() == scores[1, [1, 4, 5]].tolist()


# ---- 2. the option's values -------------------------------------------------------------------------------------------------
def test_option_values(cpu_backend, monkeypatch):
    from nvrx_straggler import Detector
    from nvrx_straggler.reporting import ReportGenerator

    for bad in (1, -2, 65, 2.0, "8", None, True):
        with pytest.raises(ValueError, match=r"score_history must be 0 \(off\) or an integer within \[2, 64\]"):
            ReportGenerator(["relative_perf_scores"], score_history=bad)
    for bad in (0, 9, -1, 2.5, "3", None, True):
        with pytest.raises(ValueError, match=r"persistence_min_reports must be an integer within \[1, score_history=8\]"):
            ReportGenerator(["relative_perf_scores"], score_history=8, persistence_min_reports=bad)
    for bad in ((0.7, 0.7, 0.7), (0.7, 0.7, 0.7, NAN), (0.7, 0.7, 0.7, math.inf), "abcd", 0.75):
        with pytest.raises(ValueError, match="persistence_thresholds must be four finite numbers"):
            ReportGenerator(["relative_perf_scores"], score_history=8, persistence_thresholds=bad)
    gen = ReportGenerator(["individual_perf_scores"], score_history=2, persistence_min_reports=2, thresholds=(0.6, 0.7, 0.8, 0.9))
    assert gen.score_history == 2 and gen.persistence_min_reports == 2 and gen.persistence_thresholds == (0.6, 0.7, 0.8, 0.9)
    gen = ReportGenerator(["relative_perf_scores"], score_history=64, persistence_thresholds=[0.5, 0.5, 0.5, 0.5])
    assert gen.persistence_min_reports == 3 and gen.persistence_thresholds == (0.5,) * 4
    off = ReportGenerator(["relative_perf_scores"], persistence_min_reports=99)  # (ignored while the option is off)
    assert off.score_history == 0 and off._history is None
    off.reset_score_history()
    # the environment variables are the Detector's defaults, read only when the argument is None
    monkeypatch.setenv("NVRX_SCORE_HISTORY", "16")
    monkeypatch.setenv("NVRX_PERSISTENCE_MIN_REPORTS", "5")
    Detector.initialize(node_name="n0")
    try:
        assert Detector.reporter.score_history == 16 and Detector.reporter.persistence_min_reports == 5
    finally:
        Detector.shutdown()
    Detector.initialize(node_name="n0", score_history=0)
    try:
        assert Detector.reporter.score_history == 0
    finally:
        Detector.shutdown()
    monkeypatch.delenv("NVRX_PERSISTENCE_MIN_REPORTS")
    monkeypatch.setenv("NVRX_SCORE_HISTORY", "2")
    Detector.initialize(node_name="n0")
    try:
        assert Detector.reporter.score_history == 2 and Detector.reporter.persistence_min_reports == 2  # (3, capped)
    finally:
        Detector.shutdown()
    monkeypatch.setenv("NVRX_SCORE_HISTORY", "many")
    with pytest.raises(ValueError, match="NVRX_SCORE_HISTORY"):
        Detector.initialize(node_name="n0")
    assert not Detector.initialized
    monkeypatch.delenv("NVRX_SCORE_HISTORY")
    Detector.initialize(node_name="n0", score_history=8, persistence_min_reports=4, persistence_thresholds=(0.6,) * 4)
    try:
        r = Detector.reporter
        assert (r.score_history, r.persistence_min_reports, r.persistence_thresholds) == (8, 4, (0.6,) * 4)
    finally:
        Detector.shutdown()
    Detector.initialize(node_name="n0")
    try:
        assert Detector.reporter.score_history == 0
    finally:
        Detector.shutdown()


def test_option_needs_a_backend_with_score_history():
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator
    from oracle_backend import OracleBackend

    backend.set_backend(OracleBackend())
    try:
        with pytest.raises(RuntimeError, match="no score history"):
            ReportGenerator(["relative_perf_scores"], score_history=8)
        ReportGenerator(["relative_perf_scores"], score_history=0)
    finally:
        backend.set_backend(None)


# ---- 3. off by default: nothing is called -----------------------------------------------------------------------------------
@pytest.mark.parametrize("emulate_fused,asynchronous", [(False, False), (True, False), (True, True)])
def test_default_is_off_and_calls_nothing(emulate_fused, asynchronous):
    from nvrx_straggler import Statistic as S
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator

    be = CountingHistoryBackend(emulate_fused=emulate_fused)
    backend.set_backend(be)
    try:
        gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=True, node_name="n",
                              asynchronous=asynchronous)
        summ = {S.MIN: 1.0, S.MAX: 2.0, S.MED: 1.5, S.AVG: 1.5, S.STD: 0.1, S.NUM: 4}
        rep = gen.generate_report({"sec": summ}, {"k": summ})
        nobody = {"straggler_gpus_relative": set(), "straggler_gpus_individual": set(), "straggler_sections_relative": {},
                  "straggler_sections_individual": {}}
        assert rep.score_history() == {} and pickle.loads(pickle.dumps(rep)).score_history() == {}
        assert rep.identify_persistent_stragglers() == nobody and rep.identify_persistent_stragglers(5) == nobody
        rings = be.make_rings(1, 8, 16)
        rows = {"sec": rings.row_for(0, "sec")}
        for i in range(3):
            rings.push_many(rows["sec"], [5.0 + i, 6.0])
            rep = gen.generate_report_from_rings(rings, rows, {})
            rings.reset()
            assert rep.score_history() == {}
        assert gen._ring_plan is not None and be.history_calls == 0
        gen.close()
    finally:
        backend.set_backend(None)


# ---- 4. the headline scenario -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("emulate_fused", [False, True])
def test_one_slow_window_flags_nobody_and_a_rank_that_stays_slow_is_flagged_at_its_third_report(emulate_fused):
    from nvrx_straggler import backend

    hw = history_workers
    be = HistoryOracleBackend(emulate_fused=emulate_fused)
    backend.set_backend(be)
    try:
        reports = hw.run_scenario(be, score_history=8, persistence_min_reports=3)
    finally:
        backend.set_backend(None)
    assert be.history_calls == hw.REPORTS and [a[3] for a in be.history_args] == list(range(hw.REPORTS))
    assert all(a[:3] == (0, hw.RANKS, len(hw.SECTIONS)) for a in be.history_args)
    assert all(h.reads == 0 for h in be.history_handles)  # generate_report reads nothing
    for i, rep in enumerate(reports):
        single, persistent = hw.ranks_of(rep.identify_stragglers()), hw.ranks_of(rep.identify_persistent_stragglers())
        # per-report flagging: rank 2 once, rank 5 from report 10
        assert single == ([hw.ONCE_RANK] if i == hw.ONCE_REPORT else [hw.STAYS_RANK] if i >= hw.STAYS_FROM else []), i
        # a streak of 3: never rank 2, rank 5 from report 12 on
        assert persistent == ([hw.STAYS_RANK] if i >= hw.STAYS_FROM + 2 else []), i
        assert hw.ranks_of(rep.identify_persistent_stragglers(1)) == single  # a streak of one is the report's own flag
        t = rep.score_history()
        json.dumps(t)
        assert t["depth"] == min(i + 1, 8) and t["capacity"] == 8 and t["min_reports"] == 3 and t["thresholds"] == (0.75,) * 4
        assert "gpu_individual" not in t and "section_individual" not in t  # (a family that was not computed)
        assert sorted(t["gpu_relative"]) == list(range(hw.RANKS)) and sorted(t["section_relative"]) == sorted(hw.SECTIONS)
        assert all(rec["present"] == 0 and math.isnan(rec["latest"]) for rec in t["gpu_relative"].values())  # (no kernels)
        for name in hw.SECTIONS:
            now = rep.section_relative_perf_scores[name]
            for r, rec in t["section_relative"][name].items():
                assert rec["latest"] == now[r] and rec["present"] == t["depth"] and rec["worst"] <= rec["median"] <= rec["best"]
            stays = t["section_relative"][name][hw.STAYS_RANK]
            assert stays["streak"] == min(max(i - hw.STAYS_FROM + 1, 0), 8) == stays["below"]
            once = t["section_relative"][name][hw.ONCE_RANK]
            assert once["streak"] == (1 if i == hw.ONCE_REPORT else 0)
            assert once["below"] == (1 if hw.ONCE_REPORT <= i < hw.ONCE_REPORT + 8 else 0)
            # 1 / 1.45 = 0.69 against the FASTEST rank's median, which 1 % noise puts a little below 1000: [0.66, 0.70]
            if i >= hw.STAYS_FROM + 3:
                assert 0.66 <= stays["median"] <= 0.70, (i, stays)  # the median of the last 8 reports, from report 13 on
            elif i >= hw.STAYS_FROM:
                assert stays["median"] > 0.9 and 0.66 <= stays["worst"] <= 0.70
    # the records are the restatement's on the reports' own scores
    hist, S = fresh(hw.RANKS, 64, 8), len(hw.SECTIONS)
    for i, rep in enumerate(reports):
        scores = np.full((hw.RANKS, 2 + 2 * S), np.nan, dtype=np.float32)
        for s, name in enumerate(hw.SECTIONS):  # (ids in the order the names were first seen)
            scores[:, 2 + S + s] = [rep.section_relative_perf_scores[name][r] for r in range(hw.RANKS)]
        rec = history_step(hist, scores, S, 0, hw.RANKS, 8, i)
        t = rep.score_history()
        for s, name in enumerate(hw.SECTIONS):
            for r in range(hw.RANKS):
                assert t["section_relative"][name][r] == as_dicts(rec[r, 1, 1 + s]), (i, name, r)


# ---- 5. new sections, growth, restart ---------------------------------------------------------------------------------------
def test_a_section_that_appears_later_has_a_history_of_its_own_and_old_columns_keep_theirs(cpu_backend):
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=True, node_name="n",
                          score_history=4, persistence_min_reports=2)
    rings = cpu_backend.make_rings(2, 80, 16)
    rows = {"old": rings.row_for(0, "old")}
    seen = []
    for i in range(9):
        if i == 5:
            rows = dict(rows, new=rings.row_for(0, "new"))
        if i == 7:  # 65 section ids: past the first capacity of 64
            rows = dict(rows, **{f"extra{k}": rings.row_for(0, f"extra{k}") for k in range(63)})
        for name, row in rows.items():
            rings.push_many(row, np.full(5, 10.0, dtype=np.float32), lr=0)
            rings.push_many(row, np.full(5, 20.0 if name == "old" else 10.0, dtype=np.float32), lr=1)  # rank 1: 0.5 on "old"
        rep = gen.generate_report_from_rings(rings, rows, {}, local_ranks=2)
        rings.reset()
        t = rep.score_history()
        seen.append(t)
        assert t["depth"] == min(i + 1, 4)
        old = t["section_relative"]["old"]
        assert old[1] == {"latest": 0.5, "median": 0.5, "worst": 0.5, "best": 0.5, "streak": t["depth"], "below": t["depth"],
                          "present": t["depth"]}
        assert old[0]["streak"] == 0 and old[0]["present"] == t["depth"] and old[0]["latest"] == 1.0
        assert ("new" in t["section_relative"]) == (i >= 5)
        if i >= 5:
            new = t["section_relative"]["new"][1]
            assert new["present"] == min(i - 5 + 1, 4) and new["streak"] == 0 and new["latest"] == 1.0  # the reports since
        if i >= 7:
            assert len(t["section_relative"]) == 65 and t["section_relative"]["extra62"][0]["present"] == i - 7 + 1
        assert hw_ranks(rep.identify_persistent_stragglers()) == ([1] if i >= 1 else [])
        assert t["section_individual"]["old"][1]["latest"] == 1.0  # (its own best median so far: the same every window)
    st = gen._history
    assert cpu_backend.history_grown == 1 and st.S_cap == 128 and st.hist.shape == (2, 2, 129, 16) and st.n_before == 9
    assert [a[2] for a in cpu_backend.history_args] == [1] * 5 + [2] * 2 + [65] * 2
    # reset_score_history: the next report starts a new history; reports handed out keep theirs
    gen.reset_score_history()
    assert st.hist is None and st.n_before == 0
    for name, row in rows.items():
        rings.push_many(row, np.full(5, 10.0, dtype=np.float32), lr=0)
        rings.push_many(row, np.full(5, 20.0, dtype=np.float32), lr=1)
    t = gen.generate_report_from_rings(rings, rows, {}, local_ranks=2).score_history()
    assert t["depth"] == 1 and t["section_relative"]["old"][1]["streak"] == 1 and st.n_before == 1
    assert seen[-1]["depth"] == 4
    gen.close()


def hw_ranks(found):
    return history_workers.ranks_of(found)


def test_another_rank_range_starts_the_history_again(cpu_backend):
    from nvrx_straggler.backend import ScoreHistory

    st = ScoreHistory(17)
    assert (st.depth, st.stride, st.n_before, st.hist) == (17, 32, 0, None)
    assert [ScoreHistory.capacity(s) for s in (0, 1, 64, 65, 128, 129)] == [64, 64, 64, 128, 128, 192]
    ws = cpu_backend.workspace(4, 0, 1)
    ws.scores[:] = 0.5
    cpu_backend.score_history(ws, st, 0, 4)
    cpu_backend.score_history(ws, st, 0, 4)
    assert st.n_before == 2 and st.ranks == (0, 4) and st.hist.shape == (4, 2, 65, 32)
    h = cpu_backend.score_history(ws, st, 1, 2)
    assert st.n_before == 1 and st.ranks == (1, 2) and st.hist.shape[0] == 2 and (h.records()[..., 7] == 1).all()


# ---- 6. lifetime and pickling -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("emulate_fused,asynchronous", [(False, False), (True, False), (True, True)])
def test_a_held_report_keeps_its_history_and_reports_travel(emulate_fused, asynchronous):
    from nvrx_straggler import Statistic as S
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator

    be = HistoryOracleBackend(emulate_fused=emulate_fused)
    backend.set_backend(be)
    try:
        gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=True, node_name="n",
                              score_history=8, persistence_min_reports=2, asynchronous=asynchronous)
        rings = be.make_rings(1, 8, 16)
        kernel_rows, section_rows = {"gemm": rings.row_for(1, "gemm")}, {"sec": rings.row_for(0, "sec")}
        held = []
        for w in range(5):
            v = np.arange(1, 12, dtype=np.float32) * (w + 1)  # every window slower: the individual scores fall
            rings.push_many(kernel_rows["gemm"], v)
            rings.push_many(section_rows["sec"], v + 0.5)
            held.append(gen.generate_report_from_rings(rings, section_rows, kernel_rows))
            rings.reset()
        assert be.history_calls == 5 and all(h.reads == 0 for h in be.history_handles)
        for w in (2, 4, 3, 0, 1):  # a report read after the next two were issued is still its own
            t = held[w].score_history()
            assert be.history_handles[w].reads == 1
            assert t["depth"] == w + 1 and t["gpu_relative"][0] == {"latest": 1.0, "median": 1.0, "worst": 1.0, "best": 1.0,
                                                                     "streak": 0, "below": 0, "present": w + 1}
            gi, si = t["gpu_individual"][0], t["section_individual"]["sec"][0]
            assert gi["latest"] == float(np.float32(1.0 / (w + 1))) == gi["worst"] and gi["best"] == 1.0
            assert gi["streak"] == gi["below"] == w and gi["present"] == w + 1  # 1, 1/2, 1/3 ...: below 0.75 from the second on
            assert si["streak"] == w and si["latest"] == held[w].section_individual_perf_scores["sec"][0]
            assert hw_ranks(held[w].identify_persistent_stragglers()) == ([0] if w >= 2 else [])
            assert held[w].score_history() == t and be.history_handles[w].reads == 1
            for clone in (pickle.loads(pickle.dumps(held[w])), copy.deepcopy(held[w])):
                assert json.dumps(clone.score_history()) == json.dumps(t)
                assert clone.identify_persistent_stragglers() == held[w].identify_persistent_stragglers()
        t = held[0].score_history()
        t["gpu_relative"].clear()
        t["section_individual"]["sec"][0]["streak"] = 99
        assert held[0].score_history()["gpu_relative"] and held[0].score_history()["section_individual"]["sec"][0]["streak"] == 0
        with pytest.raises(ValueError, match="min_reports"):
            held[0].identify_persistent_stragglers(0)
        # the dict-input path goes through the same score kernel: it appends to the same history
        summ = {S.MIN: 1.0, S.MAX: 2.0, S.MED: 1.5, S.AVG: 1.5, S.STD: 0.1, S.NUM: 4}
        t = gen.generate_report({"sec": summ}, {"gemm": summ}).score_history()
        assert t["depth"] == 6 and t["section_relative"]["sec"][0]["present"] == 6 and be.history_calls == 6
        gen.close()
    finally:
        backend.set_backend(None)


# ---- 7. gloo ranks: who holds a history, and no further collective ------------------------------------------------------------
@pytest.mark.parametrize("gather_on_rank0", [True, False])
def test_the_option_adds_no_collective_and_covers_the_reports_ranks(gather_on_rank0):
    world = 2
    on = run_ranks(history_workers.ring_reports_recorded, world, timeout=300, gather_on_rank0=gather_on_rank0, history=8)
    off = run_ranks(history_workers.ring_reports_recorded, world, timeout=300, gather_on_rank0=gather_on_rank0, history=0)
    for r in range(world):
        assert on[r]["calls"] == off[r]["calls"], r
        assert off[r]["history_calls"] == 0 and all(e["history"] in (None, {}) for e in off[r]["reports"])
        holds = r == 0 or not gather_on_rank0
        # one step per report a rank holds: the report that meets a new name is assembled once, after its second score round
        assert on[r]["history_calls"] == (6 if holds else 0), on[r]["history_calls"]
        want = (0, world) if gather_on_rank0 else (r, 1)
        assert [a[:2] for a in on[r]["history_args"]] == [want] * (6 if holds else 0)
        assert [a[3] for a in on[r]["history_args"]] == list(range(6 if holds else 0))  # n_before: once per report
        for i, entry in enumerate(on[r]["reports"]):
            if not holds:
                assert entry["history"] is None
                continue
            t = entry["history"]
            covered = list(range(world)) if gather_on_rank0 else [r]
            assert entry["pickled_same"] and t["depth"] == i + 1
            assert sorted(t["gpu_relative"]) == sorted(t["gpu_individual"]) == covered
            shown = sorted(t["section_relative"])
            assert shown[:2] == ["s0", "s1"] and ("s_new" in shown) == (i >= 2 and (gather_on_rank0 or r == world - 1))
            if "s_new" in shown:
                assert all(rec["present"] <= i - 2 + 1 for rec in t["section_relative"]["s_new"].values())
            # rank 1 is e^0.4 = 1.5 x slower throughout: 0.67, flagged in every report, persistent from the second on
            if 1 in covered:
                assert t["section_relative"]["s0"][1]["streak"] == i + 1 and 1 in entry["flagged"]
                assert (1 in entry["persistent"]) == (i >= 1)
            assert 0 not in entry["persistent"]


# ---- 8. next to everything else a report can carry: the same reports ------------------------------------------------------------
@pytest.mark.parametrize("emulate_fused,asynchronous", [(False, False), (True, False), (True, True)])
def test_reports_with_every_follow_up_say_the_same_with_and_without_the_history(emulate_fused, asynchronous):
    import row_family_script as script
    from nvrx_straggler import backend

    everything = dict(script.OPTIONS, kernel_attribution=2, robust_scores=True, robust_min_ranks=2)

    def run(**extra):
        be = HistoryOracleBackend(emulate_fused=emulate_fused)
        backend.set_backend(be)
        try:
            gen, rings, rows = script.make(be, kernels=("beat",), asynchronous=asynchronous, **everything, **extra)
            out = []
            for w in range(4):
                rep = script.report(gen, rings, rows, kernels=("beat",), window=w)
                out.append({"flagged": repr(rep.identify_stragglers()), "rel": rep.section_relative_perf_scores,
                            "gpu": rep.gpu_relative_perf_scores, "explain": rep.explain_gpu_scores(), "robust": rep.robust_scores(),
                            "tail": rep.tail_scores(), "onset": rep.onset_scores(), "period": rep.period_scores(),
                            "episode": rep.episode_scores(), "history": rep.score_history()})
            gen.close()
            return out, be
        finally:
            backend.set_backend(None)

    off, be_off = run()
    on, be_on = run(score_history=8, persistence_min_reports=2)
    assert be_off.history_calls == 0 and be_on.history_calls == 4
    for a, b in zip(off, on):
        assert a["history"] == {} and b["history"]["depth"] >= 1
        for key in a:
            if key != "history":
                assert script.same(a[key], b[key]), key
    for counter in ("score_calls", "attribute_calls", "robust_calls", "episode_score_calls", "episode_local_calls"):
        assert getattr(be_on, counter) == getattr(be_off, counter), counter


# ---- 9. the lane declines ---------------------------------------------------------------------------------------------------
def test_lane_declines_while_the_option_is_on():
    from types import SimpleNamespace

    from nvrx_straggler import straggler

    class Reached(Exception):
        pass

    class Manager:
        is_initialized = True

        @property
        def cupti_ext(self):
            raise Reached  # what _Lane.build asks for right after its option checks

    def det(depth):
        reporter = SimpleNamespace(_ring_plan=SimpleNamespace(fused=True, ws=None), world_size=1, _exchanged=lambda: True,
                                   _direct=None, asynchronous=False, kernel_attribution=0, tail_q_ppm=0, robust_scores=False,
                                   score_history=depth)
        rings = SimpleNamespace(lib=SimpleNamespace(nvrx_window_report=object()))
        return SimpleNamespace(_rings=rings, reporter=reporter, _cupti_manager=Manager(), _pending_region_switch=None)

    with pytest.raises(Reached):
        straggler._Lane.build(det(0))
    assert straggler._Lane.build(det(8)) is None


# ---- 10. the Lightning callback ---------------------------------------------------------------------------------------------
def _scripted_history(streaks, m):
    def rec(k):
        return {"latest": 0.6 if k else 0.95, "median": 0.9, "worst": 0.6, "best": 0.97, "streak": k, "below": k, "present": 8}

    return {"depth": 8, "capacity": 8, "min_reports": m, "thresholds": (0.7, 0.75, 0.7, 0.75),
            "gpu_relative": {r: rec(streaks.get(r, 0)) for r in range(8)},
            "gpu_individual": {r: rec(0) for r in range(8)}, "section_relative": {}, "section_individual": {}}


def test_callback_halts_at_the_third_flagged_report_in_a_row_and_not_at_a_single_one(monkeypatch):
    import callback_script
    import nvrx_straggler
    from nvidia_resiliency_ext.ptl_resiliency import StragglerDetectionCallback
    from nvrx_straggler.reporting import Report

    healthy, slow3 = callback_script._scores(8), callback_script._scores(8, low=[3])
    base = {k: v for k, v in callback_script.reports(8)[1].items() if not k.startswith("gpu_")}
    # (relative scores, streak of rank 3): one slow window, two healthy ones, then three slow ones in a row
    sequence = [(slow3, 1), (healthy, 0), None, (healthy, 0), (slow3, 1), (slow3, 2), (slow3, 3), (healthy, 0)]

    def scripted(n_ranks):
        return [None if e is None else dict(base, gpu_relative_perf_scores=e[0], gpu_individual_perf_scores=healthy,
                                            history=_scripted_history({3: e[1]}, 3)) for e in sequence]

    def make_report(history=None, **fields):
        rep = Report(**fields)
        rep.__dict__["_history"] = history
        return rep

    monkeypatch.setattr(callback_script, "reports", scripted)
    monkeypatch.setitem(callback_script.CONFIGS, "persist3", dict(callback_script.CONFIGS["print2_log_stop"], min_consecutive_reports=3))
    got = callback_script.drive(StragglerDetectionCallback, nvrx_straggler, make_report,
                                ("persist3", "persist3", 8, 0, False, False, False))
    assert got["initialize_calls"] == [dict(scores_to_compute=["relative_perf_scores", "individual_perf_scores"],
                                            gather_on_rank0=True, profiling_interval=1, report_time_interval=1.0, score_history=8,
                                            persistence_min_reports=3, persistence_thresholds=[0.7, 0.75, 0.7, 0.75])]
    its = got["iterations"]
    assert len(its) == len(sequence)
    warned = [any(level == "WARNING" for level, _ in it["records"]) for it in its]
    assert warned == [False] * 6 + [True, False]
    assert [it["should_stop"] for it in its] == [False] * 6 + [True, True]
    text = [m for level, m in its[6]["records"] if level == "WARNING"]
    assert text == ["STRAGGLER DETECTION WARNING: Some GPUs have worse relative performance for 3 consecutive reports. "
                    "Affected ranks: {StragglerId(rank=3, node='node0')}"]
    # every report's scores are still printed and logged, flagged or not
    for i, e in enumerate(sequence):
        if e is not None:
            assert any("GPU relative performance" in m for _, m in its[i]["records"]) and len(its[i]["log_dict"]) == 2
            assert any("Score=0.61" in m for _, m in its[i]["records"]) == (e[0] is slow3)

    # min_consecutive_reports=1, given or not: the initialize call and the transcript of today
    monkeypatch.undo()
    monkeypatch.setitem(callback_script.CONFIGS, "explicit1", dict(callback_script.CONFIGS["print2_log_stop"], min_consecutive_reports=1))
    plain = callback_script.drive(StragglerDetectionCallback, nvrx_straggler, Report, callback_script.SCENARIOS[0])
    given = callback_script.drive(StragglerDetectionCallback, nvrx_straggler, Report,
                                  ("rank0_8ranks", "explicit1", 8, 0, False, False, False))
    assert json.dumps(dict(given, config=None), sort_keys=True) == json.dumps(dict(plain, config=None), sort_keys=True)
    assert given["initialize_calls"] == [dict(scores_to_compute=["relative_perf_scores", "individual_perf_scores"],
                                              gather_on_rank0=True, profiling_interval=1, report_time_interval=1.0)]
    for bad in (0, 65, 2.0, True, None):
        with pytest.raises(ValueError, match="min_consecutive_reports"):
            StragglerDetectionCallback(**dict(callback_script.CONFIGS["quiet_rel_only"], min_consecutive_reports=bad))


# ---- 11. the C entry points check their arguments before any device is touched ------------------------------------------------
def test_entry_points_check_their_arguments_without_a_device():
    import os
    import re

    from nvrx_straggler import _native

    lib = _native.load()
    assert {"nvrx_score_history", "nvrx_report_history"} <= {name for name, _, _ in _native.SYMBOLS}
    assert lib.nvrx_abi_version() == 2 and lib.nvrx_report_desc_size() == ctypes.sizeof(_native.ReportDesc)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nvrx_straggler.h")).read()
    assert int(re.search(r"#define NVRX_HISTORY_MAX_DEPTH (\d+)", header).group(1)) == _native.HISTORY_MAX_DEPTH == 64
    assert re.search(r"#define NVRX_ABI_VERSION 2\b", header) and not re.search(r"NVRX_HISTORY\w*_PLANES", header)
    assert "#define NVRX_HISTORY_STRIDE(H) ((H) <= 16 ? 16 : (H) <= 32 ? 32 : 64)" in header
    assert [_native.history_stride(h) for h in (2, 16, 17, 32, 33, 64)] == [16, 16, 32, 32, 64, 64] == [stride(h) for h in (2, 16, 17, 32, 33, 64)]
    assert _native.history_words(8, 64) == 8 * 2 * 65 * 8 and _native.history_floats(8, 64, 17) == 8 * 2 * 65 * 32
    fake = ctypes.c_void_p(4096)
    thr = (ctypes.c_double * 4)(0.75, 0.75, 0.75, 0.75)

    def step(scores=fake, R=8, S=2, first=0, n=8, hist=fake, cap=64, H=8, before=0, thresholds=thr, out=fake):
        return lib.nvrx_score_history(scores, R, S, first, n, hist, cap, H, before, thresholds, out, None)

    for H in (1, 0, -4, 65, 1000):
        assert step(H=H) == _native.ERR_RANGE and b"depth" in lib.nvrx_last_error()
    assert step(R=0) == _native.ERR_INVALID and step(S=-1) == _native.ERR_INVALID and b"shape" in lib.nvrx_last_error()
    assert step(S=65) == _native.ERR_INVALID and b"S_cap" in lib.nvrx_last_error()
    assert step(first=7, n=2) == _native.ERR_INVALID and b"outside the scores" in lib.nvrx_last_error()
    assert step(first=-1) == _native.ERR_INVALID and step(n=0) == _native.ERR_INVALID and step(n=9) == _native.ERR_INVALID
    assert step(scores=None) == _native.ERR_INVALID and step(hist=None) == _native.ERR_INVALID and step(out=None) == _native.ERR_INVALID
    assert b"null" in lib.nvrx_last_error()
    assert step(hist=ctypes.c_void_p(4100)) == _native.ERR_INVALID and b"aligned" in lib.nvrx_last_error()
    assert step(out=ctypes.c_void_p(4104)) == _native.ERR_INVALID and step(scores=ctypes.c_void_p(4098)) == _native.ERR_INVALID
    for bad in (NAN, math.inf, -math.inf):
        assert step(thresholds=(ctypes.c_double * 4)(0.75, bad, 0.75, 0.75)) == _native.ERR_INVALID
        assert b"thresholds[1]" in lib.nvrx_last_error()

    desc = _native.ReportDesc()
    desc.R, desc.K, desc.S = 8, 8, 2

    def report(ctx=fake, d=ctypes.byref(desc), first=0, n=8, hist=fake, cap=64, H=8, before=3, thresholds=None, out=fake):
        return lib.nvrx_report_history(ctx, d, first, n, hist, cap, H, before, thresholds, out)

    assert report(ctx=None) == _native.ERR_INVALID and report(d=None) == _native.ERR_INVALID
    assert report(H=1) == _native.ERR_RANGE and report(H=65) == _native.ERR_RANGE
    assert report(first=1) == _native.ERR_INVALID and report(n=0) == _native.ERR_INVALID and report(cap=1) == _native.ERR_INVALID
    assert report(hist=None) == _native.ERR_INVALID and report(out=ctypes.c_void_p(4104)) == _native.ERR_INVALID
    assert report(thresholds=(ctypes.c_double * 4)(NAN, 0.75, 0.75, 0.75)) == _native.ERR_INVALID
