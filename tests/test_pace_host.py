"""Pace scores, host side, on the CPU checker backend (tests/pace_oracle_backend.py): the NumPy restatement against a
brute-force sort, the five scenarios of the feature's sketch (8 ranks x 120 kernels, seed 2026) through ReportGenerator, the
option's plumbing through ReportGenerator / Detector / Report / the Lightning callback, all three attachment sites, that the
option adds no collective on gloo ranks and no backend call when off, lifetime and pickling, and the argument checks of the two
C entry points (callable without a device).

Bounds: everything here runs on the restatement itself, so records are compared exactly."""
import copy
import ctypes
import json
import math
import pickle
import struct

import numpy as np
import pytest

import pace_workers
from mp_util import run_ranks
from pace_oracle_backend import CountingPaceBackend, PaceOracleBackend, pace_scores_table


@pytest.fixture
def cpu_backend():
    from nvrx_straggler import backend

    be = PaceOracleBackend()
    backend.set_backend(be)
    try:
        yield be
    finally:
        backend.set_backend(None)


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def _key(x):
    """f2key in plain Python, on the f32 bit pattern."""
    u = _bits(x)
    return (u ^ 0xFFFFFFFF) if u >> 31 else (u | 0x80000000)


def _brute(T, K, S, first, n, min_ranks):
    """The contract with Python lists and ``sorted``: ``(cols, recs)`` as lists of tuples (floats as bit patterns)."""
    KS = K + S
    NAN = 0x7FC00000
    cols = []
    for c in range(KS):
        present = [float(T[r, c]) for r in range(T.shape[0]) if T[r, c] >= 0]
        if not present:
            cols.append((NAN, 0, 0, 0, None))
            continue
        ctr = sorted(present, key=_key)[(len(present) - 1) >> 1]
        cols.append((_bits(ctr) if len(present) >= min_ranks else NAN, len(present), sum(_key(v) > _key(ctr) for v in present),
                     sum(_key(v) < _key(ctr) for v in present), ctr if len(present) >= min_ranks else None))
    recs = []
    for r in range(first, first + n):
        for lo, hi in ((0, K), (K, KS)):
            qs, columns, slower, faster = [], 0, 0, 0
            for c in range(lo, hi):
                v, ctr = float(T[r, c]), cols[c][4]
                if not v >= 0 or ctr is None:
                    continue
                columns += 1
                slower += _key(v) > _key(ctr)
                faster += _key(v) < _key(ctr)
                with np.errstate(invalid="ignore", divide="ignore"):
                    q = float(np.float32(np.float64(ctr) / np.float64(v)))  # (the IEEE quotient; the sort is what is brute here)
                if q == q:
                    qs.append(q)
            if not qs:
                recs.append((NAN, NAN, columns, slower, faster))
                continue
            pace = sorted(qs, key=_key)[(len(qs) - 1) >> 1]
            with np.errstate(invalid="ignore"):
                devs = [int(np.abs(np.float32(q) - np.float32(pace)).view(np.uint32)) & 0x7FFFFFFF for q in qs]
            recs.append((_bits(pace), sorted(devs)[(len(devs) - 1) >> 1], columns, slower, faster))
    return [c[:4] for c in cols], recs


def _small_table(rng, R, K, S):
    KS = K + S
    T = np.zeros((R, 2 * KS + K + 1), dtype=np.float32)
    T[:, :KS] = rng.choice(np.array([0.0, 1.0, 2.0, 3.0, 4.0, 6.0, np.inf, -1.0, np.nan], dtype=np.float32), (R, KS),
                           p=[0.05, 0.2, 0.2, 0.15, 0.1, 0.1, 0.05, 0.1, 0.05])
    T[:, 2 * KS : 2 * KS + K] = rng.integers(1, 50, (R, K))
    return T


# ---- 1. the restatement against a brute-force sort ---------------------------------------------------------------------------
@pytest.mark.parametrize("R,K,S,min_ranks", [(1, 3, 0, 1), (2, 2, 2, 2), (5, 4, 3, 2), (6, 0, 5, 3), (7, 9, 1, 4), (9, 6, 6, 1)])
def test_restatement_against_a_brute_force_sort(R, K, S, min_ranks):
    rng = np.random.default_rng(R * 100 + K * 10 + S)
    for _ in range(20):
        T = _small_table(rng, R, K, S)
        first = int(rng.integers(0, R))
        n = int(rng.integers(1, R - first + 1))
        cols, recs, _ = pace_scores_table(T, K, S, first, n, min_ranks)
        want_cols, want_recs = _brute(T, K, S, first, n, min_ranks)
        assert [tuple(c) for c in cols.tolist()] == want_cols
        assert [tuple(x[:5]) for x in recs.reshape(-1, 8).tolist()] == want_recs


def test_restatement_on_a_hand_worked_table():
    K, S = 3, 1
    T = np.zeros((4, 2 * (K + S) + K + 1), dtype=np.float32)
    T[:, 0] = [10.0, 10.0, 20.0, 40.0]   # lower median 10: rank 2 at 0.5, rank 3 at 0.25
    T[:, 1] = [8.0, 4.0, 8.0, -1.0]      # three present: median 8
    T[:, 2] = [1.0, -1.0, -1.0, 2.0]     # two present: below min_ranks = 3
    T[:, 3] = [5.0, 5.0, 5.0, 5.0]
    T[:, 8:11] = [[1.0, 2.0, 3.0]] * 4   # weights
    cols, recs, _ = pace_scores_table(T, K, S, min_ranks=3)
    f = recs.view(np.float32)
    assert cols[:, 1:].tolist() == [[4, 2, 0], [3, 0, 1], [2, 1, 0], [4, 0, 0]]
    assert cols.view(np.float32)[[0, 1, 3], 0].tolist() == [10.0, 8.0, 5.0] and cols[2, 0] == 0x7FC00000
    # rank 2: quotients {0.5, 1.0} -> lower median 0.5, deviations {0, 0.5} -> 0; slower in one of two columns
    assert f[2, 0, :2].tolist() == [0.5, 0.0] and recs[2, 0, 2:5].tolist() == [2, 1, 0]
    assert f[2, 0, 5:].tolist() == [3.0, 1.0, 1.0 * 0.5 + 2.0 * 0.0]
    # rank 1: {1.0, 2.0} -> 1.0; faster in one column; excess 1 * 0 + 2 * (1 - 2) = -2
    assert f[1, 0, :2].tolist() == [1.0, 0.0] and recs[1, 0, 2:5].tolist() == [2, 0, 1] and f[1, 0, 7] == -2.0
    # rank 3: only column 0 (column 1 absent, column 2 not referenced)
    assert f[3, 0, :2].tolist() == [0.25, 0.0] and recs[3, 0, 2:5].tolist() == [1, 1, 0] and f[3, 0, 7] == 0.75
    assert (f[:, 1, 0] == 1.0).all() and (recs[:, 1, 2] == 1).all() and (recs[:, 1, 5:] == 0).all()  # sections: +0.0 sums


# ---- 2. the five scenarios -----------------------------------------------------------------------------------------------------
def _load(rings, rows, med):
    for lr in range(med.shape[0]):
        for k, row in enumerate(rows.values()):
            rings.push_many(row, np.full(pace_workers.SAMPLES, med[lr, k], dtype=np.float32), lr=lr)


@pytest.mark.parametrize("emulate_fused", [False, True])
@pytest.mark.parametrize("kind", pace_workers.SCENARIOS)
def test_the_five_scenarios(kind, emulate_fused):
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator

    be = PaceOracleBackend(emulate_fused=emulate_fused)
    backend.set_backend(be)
    try:
        med = pace_workers.scenario_medians(kind)
        R, K = med.shape
        gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=True, node_name="n", pace_scores=True, robust_scores=True)
        rings = be.make_rings(R, K, 256)
        rows = {f"kernel_{k:03d}": rings.row_for(1, f"kernel_{k:03d}") for k in range(K)}
        for _ in range(2):  # the general path (_assemble), then the planned one
            _load(rings, rows, med)
            rep = gen.generate_report_from_rings(rings, {}, rows, local_ranks=R)
            rings.reset()
            found = rep.identify_pace_stragglers()
            assert sorted(found) == ["straggler_gpus_relative", "straggler_section_ranks_relative"]
            assert sorted(s.rank for s in found["straggler_gpus_relative"]) == pace_workers.NAMED[kind]
            assert found["straggler_section_ranks_relative"] == set()
            assert pace_workers.ranks_named(rep.identify_stragglers()) == []
            assert pace_workers.ranks_named(rep.identify_robust_stragglers()) == []
            t = rep.pace_scores()
            json.dumps(t)
            assert t["params"] == {"min_ranks": 4, "min_columns": 8, "min_effect": 0.03, "min_breadth": 0.9}
            assert sorted(t["ranks"]) == list(range(R)) and sorted(t["kernels"]) == sorted(rows) and t["section_columns"] == {}
            slow = t["ranks"][pace_workers.SLOW_RANK]["gpu"]
            assert slow["columns"] == K and slow["breadth"] == slow["slower"] / K
            assert math.isnan(t["ranks"][0]["sections"]["pace"]) and t["ranks"][0]["sections"]["breadth"] is None
            if kind == "slow_4pct":
                # 1 / 1.04 = 0.9615; the median of 120 quotients, each with about 1 % noise, lies well within 0.5 % of it
                assert 0.956 <= slow["pace"] <= 0.967 and slow["slower"] >= 118 and slow["excess_us"] > 0
                for r in set(range(R)) - {pace_workers.SLOW_RANK}:
                    assert 0.995 <= t["ranks"][r]["gpu"]["pace"] <= 1.005
            if kind == "slow_1p5pct":
                assert 0.98 <= slow["pace"] <= 0.99 and slow["breadth"] >= 0.8  # broad, but below the effect size
            if kind == "slow_in_few":
                assert slow["pace"] >= 0.99 and slow["breadth"] < 0.7
        assert be.pace_calls == 2 and be.pace_args == [(0, R, 4)] * 2
        gen.close()
    finally:
        backend.set_backend(None)


def test_the_rule_at_its_boundaries_and_nan_never_names():
    from nvrx_straggler.reporting import Report

    def part(pace, columns, slower):
        return {"pace": pace, "spread": 0.0, "columns": columns, "slower": slower, "faster": 0,
                "breadth": slower / columns if columns else None, "total_us": 1.0, "slower_us": 1.0, "excess_us": 1.0}

    nobody = part(float("nan"), 0, 0)
    rep = Report({}, {}, {}, {}, {r: "n" for r in range(6)}, {}, {}, 0.0, True, 0)
    rep.__dict__["_pace"] = {
        "ranks": {0: {"gpu": part(0.97, 10, 9), "sections": nobody},        # exactly at all three limits
                  1: {"gpu": part(0.9700001, 10, 10), "sections": nobody},  # effect too small
                  2: {"gpu": part(0.9, 10, 8), "sections": nobody},         # not broad enough
                  3: {"gpu": part(0.9, 7, 7), "sections": nobody},          # too few columns
                  4: {"gpu": part(float("nan"), 10, 10), "sections": part(0.5, 8, 8)},
                  5: {"gpu": nobody, "sections": nobody}},
        "kernels": {}, "section_columns": {}, "params": {"min_ranks": 4, "min_columns": 8, "min_effect": 0.03, "min_breadth": 0.9}}
    found = rep.identify_pace_stragglers()
    assert {s.rank for s in found["straggler_gpus_relative"]} == {0}
    assert {s.rank for s in found["straggler_section_ranks_relative"]} == {4}
    found = rep.identify_pace_stragglers(min_effect=0.02, min_breadth=0.8, min_columns=7)
    assert {s.rank for s in found["straggler_gpus_relative"]} == {0, 1, 2, 3}
    # no minimum at all: rank 5, which has no column, is still not named (and nothing is divided by its 0 columns)
    found = rep.identify_pace_stragglers(min_effect=0.0, min_breadth=0.01, min_columns=0)
    assert {s.rank for s in found["straggler_gpus_relative"]} == {0, 1, 2, 3}
    assert {s.rank for s in found["straggler_section_ranks_relative"]} == {4}


# ---- 3. the option's values -------------------------------------------------------------------------------------------------
def test_option_values(cpu_backend, monkeypatch):
    from nvrx_straggler import Detector
    from nvrx_straggler.reporting import ReportGenerator

    for name in ("pace_min_ranks", "pace_min_columns"):
        for bad in (0, -1, 2.5, "4", None, True):
            with pytest.raises(ValueError, match=name):
                ReportGenerator(["relative_perf_scores"], pace_scores=True, **{name: bad})
    for bad in (-0.01, 1.0, float("nan"), "x", None):
        with pytest.raises(ValueError, match="pace_min_effect"):
            ReportGenerator(["relative_perf_scores"], pace_scores=True, pace_min_effect=bad)
    for bad in (0.0, -0.5, 1.01, float("nan"), "x", None):
        with pytest.raises(ValueError, match="pace_min_breadth"):
            ReportGenerator(["relative_perf_scores"], pace_scores=True, pace_min_breadth=bad)
    with pytest.raises(ValueError, match="pace_scores.*relative_perf_scores"):
        ReportGenerator(["individual_perf_scores"], pace_scores=True)
    with pytest.raises(ValueError, match="pace_scores.*relative_perf_scores"):
        Detector.initialize(scores_to_compute=["individual_perf_scores"], pace_scores=True)
    assert not Detector.initialized
    gen = ReportGenerator(["relative_perf_scores"], pace_scores=True)
    assert (gen.pace_scores, gen.pace_min_ranks, gen.pace_min_columns, gen.pace_min_effect, gen.pace_min_breadth) == (True, 4, 8, 0.03, 0.9)
    gen = ReportGenerator(["relative_perf_scores"], pace_scores=True, pace_min_ranks=1, pace_min_columns=2, pace_min_effect=0,
                          pace_min_breadth=1)
    assert (gen.pace_min_ranks, gen.pace_min_columns, gen.pace_min_effect, gen.pace_min_breadth) == (1, 2, 0.0, 1.0)
    assert not ReportGenerator(["individual_perf_scores"]).pace_scores
    # bad values are not looked at while the option is off
    assert not ReportGenerator(["relative_perf_scores"], pace_min_ranks=0).pace_scores
    # the environment variable is the Detector's default, read only when the argument is None
    for env, arg, want in (("1", None, True), ("1", False, False), ("0", None, False), (None, True, True), (None, None, False)):
        if env is None:
            monkeypatch.delenv("NVRX_PACE_SCORES", raising=False)
        else:
            monkeypatch.setenv("NVRX_PACE_SCORES", env)
        Detector.initialize(node_name="n0", **({} if arg is None else {"pace_scores": arg}))
        try:
            assert Detector.reporter.pace_scores is want, (env, arg)
        finally:
            Detector.shutdown()
    Detector.initialize(node_name="n0", pace_scores=True, pace_min_ranks=2, pace_min_columns=3, pace_min_effect=0.1, pace_min_breadth=0.5)
    try:
        gen = Detector.reporter
        assert (gen.pace_min_ranks, gen.pace_min_columns, gen.pace_min_effect, gen.pace_min_breadth) == (2, 3, 0.1, 0.5)
    finally:
        Detector.shutdown()


def test_option_needs_a_backend_with_pace_score():
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator
    from oracle_backend import OracleBackend

    backend.set_backend(OracleBackend())
    try:
        with pytest.raises(RuntimeError, match=r"no pace scores \(backend.pace_score\)"):
            ReportGenerator(["relative_perf_scores"], pace_scores=True)
        ReportGenerator(["relative_perf_scores"], pace_scores=False)
    finally:
        backend.set_backend(None)


# ---- 4. off by default: nothing is called -----------------------------------------------------------------------------------
@pytest.mark.parametrize("emulate_fused,asynchronous", [(False, False), (True, False), (True, True)])
def test_default_is_off_and_calls_nothing(emulate_fused, asynchronous):
    from nvrx_straggler import Detector
    from nvrx_straggler import Statistic as S
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator

    be = CountingPaceBackend(emulate_fused=emulate_fused)
    backend.set_backend(be)
    try:
        gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=True, node_name="n",
                              asynchronous=asynchronous)
        assert gen.pace_scores is False
        summ = {S.MIN: 1.0, S.MAX: 2.0, S.MED: 1.5, S.AVG: 1.5, S.STD: 0.1, S.NUM: 4}
        rep = gen.generate_report({"sec": summ}, {"k": summ})
        assert rep.pace_scores() == {} and pickle.loads(pickle.dumps(rep)).pace_scores() == {}
        assert rep.identify_pace_stragglers() == {"straggler_gpus_relative": set(), "straggler_section_ranks_relative": set()}
        rings = be.make_rings(1, 8, 16)
        krow, srow = rings.row_for(1, "kern"), rings.row_for(0, "sec")
        kernel_rows, section_rows = {"kern": krow}, {"sec": srow}
        for i in range(3):
            rings.push_many(krow, [1.0 + i, 2.0, 3.0])
            rings.push_many(srow, [5.0, 6.0])
            rep = gen.generate_report_from_rings(rings, section_rows, kernel_rows)
            rings.reset()
            assert rep.pace_scores() == {}
        assert gen._ring_plan is not None
        gen.close()
        Detector.initialize(scores_to_compute="all", gather_on_rank0=True, node_name="n0", asynchronous=asynchronous)
        try:
            for t in range(3):
                for name, value in (("a", 2.0 + t), ("b", 4.0)):
                    with Detector.detection_section(name, profile_cuda=False):
                        pass
                    sec = Detector.custom_sections[name]
                    sec.cpu_elapsed_times.clear()
                    sec.cpu_elapsed_times.extend(np.full(5, value, dtype=np.float32))
                assert Detector.generate_report().pace_scores() == {}
        finally:
            Detector.shutdown()
        assert be.pace_calls == 0
    finally:
        backend.set_backend(None)


# ---- 5. all three attachment sites, behind robust and peer ------------------------------------------------------------------
@pytest.mark.parametrize("emulate_fused,asynchronous", [(False, False), (True, False), (True, True)])
def test_all_three_attachment_sites(emulate_fused, asynchronous):
    from nvrx_straggler import Statistic as S
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator

    be = PaceOracleBackend(emulate_fused=emulate_fused)
    backend.set_backend(be)
    try:
        order = []
        for name in ("robust_score", "peer_score", "pace_score"):
            def spy(*a, _name=name, _inner=getattr(be, name), **kw):
                order.append(_name)
                return _inner(*a, **kw)
            setattr(be, name, spy)
        gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=True, node_name="n",
                              asynchronous=asynchronous, pace_scores=True, robust_scores=True, peer_groups="block:1",
                              peer_min_ranks=1, pace_min_columns=1)
        # (a) the dict-input report: _assemble
        summ = {S.MIN: 1.0, S.MAX: 2.0, S.MED: 1.5, S.AVG: 1.5, S.STD: 0.1, S.NUM: 4}
        t = gen.generate_report({"sec": summ}, {"gemm": summ}).pace_scores()
        assert order == ["robust_score", "peer_score", "pace_score"]
        assert t["kernels"] == {"gemm": {"center": 1.5, "ranks": 1, "above": 0, "below": 0}}
        assert t["section_columns"] == {"sec": {"center": 1.5, "ranks": 1, "above": 0, "below": 0}}
        assert t["ranks"][0]["gpu"] == {"pace": 1.0, "spread": 0.0, "columns": 1, "slower": 0, "faster": 0, "breadth": 0.0,
                                        "total_us": 6.0, "slower_us": 0.0, "excess_us": 0.0}
        assert t["ranks"][0]["sections"] == {"pace": 1.0, "spread": 0.0, "columns": 1, "slower": 0, "faster": 0, "breadth": 0.0}
        assert t["params"]["min_ranks"] == 1  # (one rank: clamped)
        # (b) ring reports: _assemble for the first, then the planned path -- stepwise, or one call through the rings
        rings = be.make_rings(1, 8, 16)
        kernel_rows = {"gemm": rings.row_for(1, "gemm")}
        section_rows = {"sec": rings.row_for(0, "sec")}
        before = be.pace_calls
        for w in range(4):
            v = np.arange(1, 12, dtype=np.float32) * (w + 1)
            rings.push_many(kernel_rows["gemm"], v)
            rings.push_many(section_rows["sec"], v[::-1] + 0.5)
            t = gen.generate_report_from_rings(rings, section_rows, kernel_rows).pace_scores()
            rings.reset()
            assert t["kernels"] == {"gemm": {"center": 6.0 * (w + 1), "ranks": 1, "above": 0, "below": 0}}
            assert t["section_columns"]["sec"]["center"] == 6.0 * (w + 1) + 0.5
            assert t["ranks"][0]["gpu"]["pace"] == 1.0 and t["ranks"][0]["gpu"]["total_us"] == float(np.float32(v.sum()))
        assert gen._ring_plan is not None and gen._ring_plan.fused == emulate_fused
        assert be.pace_calls - before == 4 and be.pace_args[-1] == (0, 1, 1)
        # the reports in front of the plan went through the backend (_assemble); the planned ones through the backend again
        # (stepwise) or through the rings' report_pace (one call)
        through_rings = be.pace_calls - order.count("pace_score")
        assert through_rings == (3 if emulate_fused else 0)
        gen.close()
    finally:
        backend.set_backend(None)


# ---- 6. no further collective; only where the rank holds a report, for the ranks it covers ---------------------------------
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("gather_on_rank0", [True, False])
def test_the_option_adds_no_collective_and_covers_the_reports_ranks(world, gather_on_rank0):
    on = run_ranks(pace_workers.ring_reports_recorded, world, timeout=300, gather_on_rank0=gather_on_rank0, pace=True)
    off = run_ranks(pace_workers.ring_reports_recorded, world, timeout=300, gather_on_rank0=gather_on_rank0, pace=False)
    for r in range(world):
        assert on[r]["calls"] == off[r]["calls"], r
        assert off[r]["pace_calls"] == 0 and all(e["pace"] in (None, {}) for e in off[r]["reports"])
        holds = r == 0 or not gather_on_rank0
        assert on[r]["pace_calls"] == (6 if holds else 0), on[r]["pace_calls"]
        want = (0, world, 2) if gather_on_rank0 else (r, 1, 2)
        assert all(a == want for a in on[r]["pace_args"]), on[r]["pace_args"]
        for entry in on[r]["reports"]:
            if not holds:
                assert entry["pace"] is None
                continue
            t = entry["pace"]
            assert entry["pickled_same"]
            assert sorted(t["ranks"]) == (list(range(world)) if gather_on_rank0 else [r])
            assert {"k0", "k1"} <= set(t["kernels"]) and "ncclDevKernel_z" not in t["kernels"]
            assert all(c["ranks"] == world for n, c in t["kernels"].items() if n in ("k0", "k1"))
            assert {"s0", "s1"} <= set(t["section_columns"])


# ---- 7. lifetime and pickling -------------------------------------------------------------------------------------------------
def test_a_held_report_keeps_its_pace_scores_and_reports_travel(cpu_backend):
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=True, node_name="n", pace_scores=True)
    rings = cpu_backend.make_rings(1, 8, 16)
    kernel_rows = {"gemm": rings.row_for(1, "gemm")}
    section_rows = {"sec": rings.row_for(0, "sec")}
    held = []
    for w in range(4):
        v = np.arange(1, 12, dtype=np.float32) * (w + 1)
        rings.push_many(kernel_rows["gemm"], v)
        rings.push_many(section_rows["sec"], v[::-1] + 0.5)
        held.append(gen.generate_report_from_rings(rings, section_rows, kernel_rows))
        rings.reset()
    assert cpu_backend.pace_calls == 4 and all(h.reads == 0 for h in cpu_backend.pace_handles)  # generate_report reads nothing
    for w in (1, 0, 3, 2):  # a report held across the next two is still its own
        t = held[w].pace_scores()
        assert cpu_backend.pace_handles[w].reads == 1
        assert t["kernels"]["gemm"]["center"] == 6.0 * (w + 1) and t["section_columns"]["sec"]["center"] == 6.0 * (w + 1) + 0.5
        assert held[w].pace_scores() == t and cpu_backend.pace_handles[w].reads == 1
        for clone in (pickle.loads(pickle.dumps(held[w])), copy.deepcopy(held[w])):
            assert json.dumps(clone.pace_scores()) == json.dumps(t)
            assert clone.identify_pace_stragglers() == held[w].identify_pace_stragglers()
            assert isinstance(clone.__dict__["_pace"], dict)  # materialised
    t = held[0].pace_scores()
    t["kernels"].clear()
    t["ranks"][0]["gpu"].clear()
    assert held[0].pace_scores()["kernels"] and held[0].pace_scores()["ranks"][0]["gpu"]


# ---- 8. the lane declines -------------------------------------------------------------------------------------------------------
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

    def det(on):
        reporter = SimpleNamespace(_ring_plan=SimpleNamespace(fused=True, ws=None), world_size=1, _exchanged=lambda: True,
                                   _direct=None, asynchronous=False, kernel_attribution=0, tail_q_ppm=0, pace_scores=on)
        rings = SimpleNamespace(lib=SimpleNamespace(nvrx_window_report=object()))
        return SimpleNamespace(_rings=rings, reporter=reporter, _cupti_manager=Manager(), _pending_region_switch=None)

    with pytest.raises(Reached):
        straggler._Lane.build(det(False))
    assert straggler._Lane.build(det(True)) is None


# ---- 9. the Lightning callback ------------------------------------------------------------------------------------------------
def test_callback_warns_of_a_rank_off_the_pace_and_never_halts_for_it(monkeypatch):
    import callback_script
    import nvrx_straggler
    from nvidia_resiliency_ext.ptl_resiliency import StragglerDetectionCallback
    from nvrx_straggler.reporting import Report

    healthy = callback_script._scores(8)
    base = {k: v for k, v in callback_script.reports(8)[1].items() if not k.startswith("gpu_")}
    sequence = [None, {5: 0.961}, None, {}, {5: 0.95, 2: 0.9}, {5: 0.985}]

    def pace_of(slow):
        def gpu(r):
            pace = slow.get(r, 1.0)
            slower = 120 if r in slow else 55
            return {"pace": pace, "spread": 0.007, "columns": 120, "slower": slower, "faster": 120 - slower,
                    "breadth": slower / 120, "total_us": 1e6, "slower_us": 1e6 * slower / 120, "excess_us": 1e6 * (1 - pace)}
        none = {"pace": float("nan"), "spread": float("nan"), "columns": 0, "slower": 0, "faster": 0, "breadth": None}
        return {"ranks": {r: {"gpu": gpu(r), "sections": dict(none)} for r in range(8)}, "kernels": {}, "section_columns": {},
                "params": {"min_ranks": 4, "min_columns": 8, "min_effect": 0.03, "min_breadth": 0.9}}

    def scripted(n_ranks):
        return [None if e is None else dict(base, gpu_relative_perf_scores=healthy, gpu_individual_perf_scores=healthy,
                                            pace=pace_of(e)) for e in sequence]

    def make_report(pace=None, **fields):
        rep = Report(**fields)
        rep.__dict__["_pace"] = pace
        return rep

    monkeypatch.setattr(callback_script, "reports", scripted)
    monkeypatch.setitem(callback_script.CONFIGS, "off_pace", dict(callback_script.CONFIGS["print2_log_stop"], warn_if_off_pace=True))
    got = callback_script.drive(StragglerDetectionCallback, nvrx_straggler, make_report,
                                ("off_pace", "off_pace", 8, 0, False, False, False))
    assert got["initialize_calls"] == [dict(scores_to_compute=["relative_perf_scores", "individual_perf_scores"],
                                            gather_on_rank0=True, profiling_interval=1, report_time_interval=1.0,
                                            pace_scores=True)]
    its = got["iterations"]
    warnings = [[m for level, m in it["records"] if level == "WARNING"] for it in its]
    assert [len(w) for w in warnings] == [0, 1, 0, 0, 1, 0]  # one warning per report that names anybody
    assert warnings[1] == ["STRAGGLER DETECTION WARNING: Some GPUs are a little slower in nearly all of their kernels (degraded "
                           "card?): rank 5 (pace 0.961, slower in 120 of 120 kernels, excess_us=39000)"]
    assert "rank 2 (pace 0.900" in warnings[4][0] and "rank 5 (pace 0.950" in warnings[4][0]
    assert [it["should_stop"] for it in its] == [False] * len(sequence) and all(it["exit"] is None for it in its)  # stop_if_detected=True

    # the default, given or not: the initialize call and the transcript of today
    monkeypatch.undo()
    monkeypatch.setitem(callback_script.CONFIGS, "explicit_off", dict(callback_script.CONFIGS["print2_log_stop"], warn_if_off_pace=False))
    plain = callback_script.drive(StragglerDetectionCallback, nvrx_straggler, Report, callback_script.SCENARIOS[0])
    given = callback_script.drive(StragglerDetectionCallback, nvrx_straggler, Report,
                                  ("rank0_8ranks", "explicit_off", 8, 0, False, False, False))
    assert json.dumps(dict(given, config=None), sort_keys=True) == json.dumps(dict(plain, config=None), sort_keys=True)
    assert given["initialize_calls"] == [dict(scores_to_compute=["relative_perf_scores", "individual_perf_scores"],
                                              gather_on_rank0=True, profiling_interval=1, report_time_interval=1.0)]
    with pytest.raises(ValueError, match="warn_if_off_pace needs calc_relative_gpu_perf"):
        StragglerDetectionCallback(**dict(callback_script.CONFIGS["print3_indiv_only_log"], warn_if_off_pace=True))


# ---- 10. header, bindings and macros agree; the C entry points check their arguments before any device is touched --------------
def test_entry_points_check_their_arguments_in_the_contracts_order_without_a_device():
    import os

    from nvrx_straggler import _native

    lib = _native.load()
    assert {"nvrx_pace_score", "nvrx_report_pace"} <= {name for name, _, _ in _native.SYMBOLS}
    assert lib.nvrx_abi_version() == 2
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nvrx_straggler.h")).read()
    assert "#define NVRX_PACE_WORDS(n_ranks, K, S) (4 * ((size_t)(K) + (S)) + 16 * (size_t)(n_ranks))" in header
    assert _native.pace_words(8, 35, 64) == 4 * 99 + 16 * 8
    flat = " ".join(header.split())
    assert ("int nvrx_pace_score(const float *d_table, int R, int K, int S, int first_rank, int n_ranks, int min_ranks, "
            "void *d_out, void *stream);") in flat
    assert ("int nvrx_report_pace(nvrx_ctx *ctx, const nvrx_report_desc *desc, int first_rank, int n_ranks, int min_ranks, "
            "void *d_out);") in flat
    fake, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)

    def score(table=fake, R=8, K=8, S=2, first=0, n=8, min_ranks=4, out=fake):
        return lib.nvrx_pace_score(table, R, K, S, first, n, min_ranks, out, None)

    assert score(R=0) == _native.ERR_INVALID and b"shape" in lib.nvrx_last_error()
    assert score(R=-1) == _native.ERR_INVALID and score(K=-1) == _native.ERR_INVALID and score(S=-1) == _native.ERR_INVALID
    assert score(R=65537, n=1) == _native.ERR_RANGE and b"ranks" in lib.nvrx_last_error()
    assert score(K=70000) == _native.ERR_RANGE and score(S=70000) == _native.ERR_RANGE and b"ids" in lib.nvrx_last_error()
    assert score(first=7, n=2) == _native.ERR_RANGE and b"outside the table" in lib.nvrx_last_error()
    assert score(first=-1) == _native.ERR_RANGE and score(n=0) == _native.ERR_RANGE and score(n=9) == _native.ERR_RANGE
    assert score(min_ranks=0) == _native.ERR_RANGE and b"min_ranks" in lib.nvrx_last_error()
    assert score(min_ranks=-3) == _native.ERR_RANGE
    assert score(table=None) == _native.ERR_INVALID and score(out=None) == _native.ERR_INVALID
    assert b"null" in lib.nvrx_last_error()
    assert score(out=odd) == _native.ERR_INVALID and b"aligned" in lib.nvrx_last_error()
    # the order of nvrx_robust_score, without floor_rel: shape, R, ids, rank range, min_ranks, pointers, alignment
    assert score(R=0, K=70000, first=-1, min_ranks=0, table=None, out=odd) == _native.ERR_INVALID and b"shape" in lib.nvrx_last_error()
    assert score(R=65537, K=70000, first=-1, min_ranks=0, table=None) == _native.ERR_RANGE and b"at most 65536" in lib.nvrx_last_error()
    assert score(K=70000, first=-1, min_ranks=0, table=None) == _native.ERR_RANGE and b"ids" in lib.nvrx_last_error()
    assert score(first=-1, min_ranks=0, table=None) == _native.ERR_RANGE and b"outside" in lib.nvrx_last_error()
    assert score(min_ranks=0, table=None, out=odd) == _native.ERR_RANGE and b"min_ranks" in lib.nvrx_last_error()
    assert score(table=None, out=odd) == _native.ERR_INVALID and b"null" in lib.nvrx_last_error()

    desc = _native.ReportDesc()
    desc.R, desc.K, desc.S = 8, 8, 2

    def report(ctx=fake, d=ctypes.byref(desc), first=0, n=8, min_ranks=4, out=fake):
        return lib.nvrx_report_pace(ctx, d, first, n, min_ranks, out)

    assert report(ctx=None) == _native.ERR_INVALID and report(d=None) == _native.ERR_INVALID
    assert report(first=1) == _native.ERR_RANGE and report(n=0) == _native.ERR_RANGE
    assert report(min_ranks=0) == _native.ERR_RANGE
    assert report(out=None) == _native.ERR_INVALID and report(out=ctypes.c_void_p(4104)) == _native.ERR_INVALID
    assert report(first=1, min_ranks=0, out=None) == _native.ERR_RANGE and b"outside" in lib.nvrx_last_error()
