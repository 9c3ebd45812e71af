"""Robust scores, host side, on the CPU checker backend (tests/robust_oracle_backend.py): the option's plumbing through
ReportGenerator / Detector / Report, the headline case of one anomalously fast rank, that the option adds no collective on
gloo ranks, all three follow-ups together, lifetime and pickling, and the argument checks of the two C entry points
(callable without a device).

Bounds: column records, section ratios and section z are compared exactly against the NumPy restatement (an actual value;
f32 products and a maximum; one f64 quotient rounded to f32); GPU slots within 2e-6 * max(1, |expected|), the project's
tolerance for the same f64 weighted mean summed in another order."""
import copy
import json
import math
import pickle

import numpy as np
import pytest

import robust_workers
from mp_util import run_ranks
from robust_oracle_backend import CountingRobustBackend, RobustOracleBackend, robust_columns, robust_scores_table

ALL_BUT_FAST = [0, 1, 2, 3, 4, 6, 7]


@pytest.fixture
def cpu_backend():
    from nvrx_straggler import backend

    be = RobustOracleBackend()
    backend.set_backend(be)
    try:
        yield be
    finally:
        backend.set_backend(None)


# ---- 1. the restatement itself, on a column worked out by hand ----------------------------------------------------------------
def test_restatement_on_a_hand_worked_column():
    K, S = 1, 1
    T = np.zeros((6, 2 * (K + S) + K + 1), dtype=np.float32)
    T[:, 0] = [10.0, 12.0, -1.0, 11.0, 30.0, np.nan]  # present: 10 12 11 30 -> lower median 11; deviations 1 1 0 19 -> 1
    T[:, 1] = [5.0, 5.0, 5.0, 5.0, 5.0, 5.0]          # all equal: mad 0, the floor decides
    T[:, 4] = [2.0, 1.0, 0.0, 1.0, 1.0, 0.0]          # kernel weights
    cols, sc = robust_scores_table(T, K, S, min_ranks=4, floor_rel=0.02)
    f = cols.view(np.float32)
    assert cols[:, 3].tolist() == [4, 6]
    assert f[0, 0] == 11.0 and f[0, 1] == 1.0 and f[0, 2] == np.float32(1.4826)
    assert f[1, 0] == 5.0 and f[1, 1] == 0.0 and f[1, 2] == np.float32(0.02) * np.float32(5.0)
    assert sc[4, 0, 0] == np.float32(11.0 / 30.0) and sc[4, 1, 0] == np.float32(19.0 / np.float64(np.float32(1.4826)))
    assert math.isnan(sc[2, 0, 0]) and math.isnan(sc[5, 1, 0])  # absent values
    assert (sc[:, 0, 1] == 1.0).all() and (sc[:, 1, 1] == 0.0).all()
    # fewer than min_ranks present values: no reference, n still written
    cols5 = robust_columns(T, K, S, 5, 0.02)
    assert cols5[0, 3] == 4 and np.isnan(cols5.view(np.float32)[0, :3]).all() and cols5[1, 3] == 6
    # floor 0 and an all-equal column: scale 0, z = 0/0 for everybody, never an error
    _, sc0 = robust_scores_table(T, K, S, min_ranks=1, floor_rel=0.0)
    assert np.isnan(sc0[:, 1, 1]).all() and (sc0[:, 0, 1] == 1.0).all()


# ---- 2. the option's values -------------------------------------------------------------------------------------------------
def test_option_values(cpu_backend, monkeypatch):
    from nvrx_straggler import Detector
    from nvrx_straggler.reporting import ReportGenerator

    for bad in (0, -1, 2.5, "4", None, True):
        with pytest.raises(ValueError, match="robust_min_ranks"):
            ReportGenerator(["relative_perf_scores"], robust_scores=True, robust_min_ranks=bad)
    for bad in (-0.01, 1.5, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match="robust_floor"):
            ReportGenerator(["relative_perf_scores"], robust_scores=True, robust_floor=bad)
    with pytest.raises(ValueError, match="robust_scores.*relative_perf_scores"):
        ReportGenerator(["individual_perf_scores"], robust_scores=True)
    with pytest.raises(ValueError, match="robust_scores.*relative_perf_scores"):
        Detector.initialize(scores_to_compute=["individual_perf_scores"], robust_scores=True)
    assert not Detector.initialized
    gen = ReportGenerator(["relative_perf_scores"], robust_scores=True)
    assert gen.robust_scores and gen.robust_min_ranks == 4 and gen.robust_floor == 0.02
    gen = ReportGenerator(["relative_perf_scores"], robust_scores=True, robust_min_ranks=1, robust_floor=0)
    assert gen.robust_min_ranks == 1 and gen.robust_floor == 0.0
    assert not ReportGenerator(["individual_perf_scores"]).robust_scores
    # the environment variable is the Detector's default, read only when the argument is None
    monkeypatch.setenv("NVRX_ROBUST_SCORES", "1")
    Detector.initialize(node_name="n0")
    try:
        assert Detector.reporter.robust_scores
    finally:
        Detector.shutdown()
    Detector.initialize(node_name="n0", robust_scores=False)
    try:
        assert not Detector.reporter.robust_scores
    finally:
        Detector.shutdown()
    monkeypatch.setenv("NVRX_ROBUST_SCORES", "0")
    Detector.initialize(node_name="n0")
    try:
        assert not Detector.reporter.robust_scores
    finally:
        Detector.shutdown()
    monkeypatch.delenv("NVRX_ROBUST_SCORES")
    Detector.initialize(node_name="n0", robust_scores=True)
    try:
        assert Detector.reporter.robust_scores
    finally:
        Detector.shutdown()


def test_option_needs_a_backend_with_robust_score():
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator
    from oracle_backend import OracleBackend

    backend.set_backend(OracleBackend())
    try:
        with pytest.raises(RuntimeError, match="no robust scores"):
            ReportGenerator(["relative_perf_scores"], robust_scores=True)
        ReportGenerator(["relative_perf_scores"], robust_scores=False)
    finally:
        backend.set_backend(None)


# ---- 3. off by default: nothing is called -----------------------------------------------------------------------------------
@pytest.mark.parametrize("emulate_fused,asynchronous", [(False, False), (True, False), (True, True)])
def test_default_is_off_and_calls_nothing(emulate_fused, asynchronous):
    from nvrx_straggler import Detector
    from nvrx_straggler import Statistic as S
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator

    be = CountingRobustBackend(emulate_fused=emulate_fused)
    backend.set_backend(be)
    try:
        gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=True, node_name="n",
                              asynchronous=asynchronous)
        assert gen.robust_scores is False
        summ = {S.MIN: 1.0, S.MAX: 2.0, S.MED: 1.5, S.AVG: 1.5, S.STD: 0.1, S.NUM: 4}
        rep = gen.generate_report({"sec": summ}, {"k": summ})
        assert rep.robust_scores() == {} and pickle.loads(pickle.dumps(rep)).robust_scores() == {}
        assert rep.identify_robust_stragglers() == {"straggler_gpus_relative": set(), "straggler_sections_relative": {}}
        rings = be.make_rings(1, 8, 16)
        krow, srow = rings.row_for(1, "kern"), rings.row_for(0, "sec")
        kernel_rows, section_rows = {"kern": krow}, {"sec": srow}
        for i in range(3):
            rings.push_many(krow, [1.0 + i, 2.0, 3.0])
            rings.push_many(srow, [5.0, 6.0])
            rep = gen.generate_report_from_rings(rings, section_rows, kernel_rows)
            rings.reset()
            assert rep.robust_scores() == {}
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
                assert Detector.generate_report().robust_scores() == {}
        finally:
            Detector.shutdown()
        assert be.robust_calls == 0
    finally:
        backend.set_backend(None)


# ---- 4. the headline case -----------------------------------------------------------------------------------------------------
def _load_scenario(rings, names, med):
    rows = {n: rings.row_for(0, n) for n in names}
    for lr in range(med.shape[0]):
        for s, n in enumerate(names):
            rings.push_many(rows[n], np.full(5, med[lr, s], dtype=np.float32), lr=lr)
    return rows


@pytest.mark.parametrize("emulate_fused", [False, True])
def test_one_fast_rank_flags_seven_of_eight_by_the_minimum_and_one_by_the_median(emulate_fused):
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator

    be = RobustOracleBackend(emulate_fused=emulate_fused)
    backend.set_backend(be)
    try:
        med = robust_workers.scenario_medians()
        names = [f"section_{s:03d}" for s in range(64)]
        gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=True, node_name="n", robust_scores=True)
        rings = be.make_rings(8, 64, 16)
        rows = _load_scenario(rings, names, med)
        exp_cols, exp = robust_scores_table(np.concatenate([med, np.full_like(med, np.nan), np.ones((8, 1), np.float32)], axis=1),
                                            0, 64, 0, 8, 4, 0.02)
        for i in range(3):  # the general path, then the planned one
            if i:
                _load_scenario(rings, names, med)
            rep = gen.generate_report_from_rings(rings, rows, {}, local_ranks=8)
            rings.reset()
            assert robust_workers.flagged(rep.identify_stragglers()) == ALL_BUT_FAST
            found = rep.identify_robust_stragglers()
            assert found["straggler_gpus_relative"] == set()  # (no kernels: the GPU slots are NaN)
            assert sorted(found["straggler_sections_relative"]) == names
            assert all({s.rank for s in v} == {robust_workers.SLOW_RANK} for v in found["straggler_sections_relative"].values())
            t = rep.robust_scores()
            json.dumps(t)
            assert t["min_ranks"] == 4 and t["floor"] == 0.02 and t["kernel_center"] == {}
            assert all(math.isnan(v) for v in t["gpu_ratio"].values()) and sorted(t["gpu_z"]) == list(range(8))
            for s, n in enumerate(names):
                assert t["ranks_with_data"][n] == 8
                assert t["section_center"][n] == float(np.sort(med[:, s])[3])  # the lower median of eight
                assert t["section_center"][n] == float(exp_cols.view(np.float32)[s, 0])
                assert t["section_spread"][n] == float(exp_cols.view(np.float32)[s, 2])
                for r in range(8):
                    ratio, z = t["section_ratio"][n][r], t["section_z"][n][r]
                    assert ratio == float(exp[r, 0, 1 + s]) and z == float(exp[r, 1, 1 + s]), (n, r)
                    if r == robust_workers.SLOW_RANK:
                        # 1 / 1.3 = 0.77, both medians within four sigma of 1 %; z is beyond the cut-off
                        assert 0.70 <= ratio <= 0.84 and z > 3.5, (n, ratio, z)
                    elif r == robust_workers.FAST_RANK:
                        assert ratio > 1.5 and z < -3.5, (n, ratio, z)
                    else:
                        assert 0.92 <= ratio <= 1.08 and z <= 3.5, (n, r, ratio, z)
        assert be.robust_calls == 3 and all(a == (0, 8, 4, 0.02) for a in be.robust_args)
        gen.close()
    finally:
        backend.set_backend(None)


# ---- 5. no further collective ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("gather_on_rank0", [True, False])
def test_the_option_adds_no_collective_and_covers_the_reports_ranks(world, gather_on_rank0):
    on = run_ranks(robust_workers.ring_reports_recorded, world, timeout=300, gather_on_rank0=gather_on_rank0, robust=True)
    off = run_ranks(robust_workers.ring_reports_recorded, world, timeout=300, gather_on_rank0=gather_on_rank0, robust=False)
    for r in range(world):
        assert on[r]["calls"] == off[r]["calls"], r
        assert off[r]["robust_calls"] == 0
        holds = r == 0 or not gather_on_rank0
        # one robust step per report a rank holds -- except that the report which meets a new name is assembled once, after
        # its second score round
        assert on[r]["robust_calls"] == (6 if holds else 0), on[r]["robust_calls"]
        want = (0, world) if gather_on_rank0 else (r, 1)
        assert all(a[:2] == want and a[2] == 2 and a[3] == 0.02 for a in on[r]["robust_args"]), on[r]["robust_args"]
    for i in range(6):
        # what every rank pushed -> medians -> the restatement on one column
        for r in range(world):
            entry = on[r]["reports"][i]
            if gather_on_rank0 and r != 0:
                assert entry["robust"] is None
                continue
            t = entry["robust"]
            assert entry["pickled_same"] and entry["explained"] == [] and entry["tails"] == []
            covered = list(range(world)) if gather_on_rank0 else [r]
            assert sorted(t["gpu_z"]) == sorted(t["gpu_ratio"]) == covered
            for key in ("section:s0", "section:s1", "kernel:k0"):
                kind, name = key.split(":")
                meds = np.array([np.sort(np.array(on[q]["reports"][i]["pushed"][key], dtype=np.float32))[
                    (len(on[q]["reports"][i]["pushed"][key]) - 1) // 2] for q in range(world)], dtype=np.float32)
                ctr = float(np.sort(meds)[(world - 1) // 2])
                if kind == "section":
                    assert t["section_center"][name] == ctr, (i, r, name)
                    for q in covered:
                        assert t["section_ratio"][name][q] == float(np.float32(np.float64(ctr) / np.float64(meds[q])))
                else:
                    # (a kernel row's MED averages the two middle samples of an even count: only its range is checked here)
                    every = np.concatenate([np.array(on[q]["reports"][i]["pushed"][key], dtype=np.float32) for q in range(world)])
                    assert every.min() <= t["kernel_center"][name] <= every.max(), (i, r, name)
                assert t["ranks_with_data"][name] == world
            assert "ncclDevKernel_z" not in t["kernel_center"]


# ---- 6. all three follow-ups together ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [1, 2])
def test_all_three_follow_ups_together(world):
    if world == 1:
        res = [robust_workers.ring_reports_recorded(0, 1, True, robust=True, kernel_attribution=2, tail_quantile=0.9)]
        from nvrx_straggler import backend

        backend.set_backend(None)
    else:
        res = run_ranks(robust_workers.ring_reports_recorded, world, timeout=300, gather_on_rank0=True, robust=True,
                        kernel_attribution=2, tail_quantile=0.9)
    assert res[0]["robust_calls"] == 6
    for entry in res[0]["reports"]:
        assert entry["pickled_same"] and entry["explained"] == ["individual", "relative"]
        assert "gpu_relative" in entry["tails"] and sorted(entry["robust"]["gpu_z"]) == list(range(world))
        assert entry["robust"]["min_ranks"] == min(2, world)


@pytest.mark.parametrize("asynchronous", [False, True])
def test_one_call_report_with_attribution_and_robust_scores(asynchronous):
    res = robust_workers.ring_reports_recorded(0, 1, True, robust=True, emulate_fused=True, asynchronous=asynchronous,
                                               kernel_attribution=2)
    from nvrx_straggler import backend

    backend.set_backend(None)
    assert res["robust_calls"] == 6
    for entry in res["reports"]:
        assert entry["explained"] == ["individual", "relative"] and entry["robust"]["gpu_z"] == {0: 0.0}
        assert entry["robust"]["gpu_ratio"] == {0: 1.0} and entry["robust"]["min_ranks"] == 1


# ---- 7. lifetime and pickling -------------------------------------------------------------------------------------------------
def test_a_held_report_keeps_its_robust_scores_and_reports_travel(cpu_backend):
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=True, node_name="n",
                          robust_scores=True)
    rings = cpu_backend.make_rings(1, 8, 16)
    kernel_rows = {n: rings.row_for(1, n) for n in ("gemm", "ncclDevKernel_y")}
    section_rows = {"sec": rings.row_for(0, "sec")}
    held = []
    for w in range(4):
        v = np.arange(1, 12, dtype=np.float32) * (w + 1)
        rings.push_many(kernel_rows["gemm"], v)
        rings.push_many(kernel_rows["ncclDevKernel_y"], v * 100)
        rings.push_many(section_rows["sec"], v[::-1] + 0.5)
        held.append(gen.generate_report_from_rings(rings, section_rows, kernel_rows))
        rings.reset()
    assert gen._ring_plan is not None and cpu_backend.robust_calls == 4
    assert all(h.reads == 0 for h in cpu_backend.robust_handles)  # generate_report reads nothing
    for w in (3, 2, 1, 0):
        t = held[w].robust_scores()
        assert cpu_backend.robust_handles[w].reads == 1
        assert t["kernel_center"] == {"gemm": 6.0 * (w + 1)} and t["section_center"] == {"sec": 6.0 * (w + 1) + 0.5}
        assert t["gpu_ratio"] == {0: 1.0} and t["gpu_z"] == {0: 0.0} and t["min_ranks"] == 1  # (one rank: clamped)
        assert t["section_ratio"] == {"sec": {0: 1.0}} and t["section_z"] == {"sec": {0: 0.0}}
        assert t["ranks_with_data"] == {"gemm": 1, "sec": 1}
        assert held[w].robust_scores() == t and cpu_backend.robust_handles[w].reads == 1
        for clone in (pickle.loads(pickle.dumps(held[w])), copy.deepcopy(held[w])):
            assert json.dumps(clone.robust_scores()) == json.dumps(t)
            assert clone.identify_robust_stragglers() == held[w].identify_robust_stragglers()
    t = held[0].robust_scores()
    t["kernel_center"].clear()
    t["section_z"]["sec"].clear()
    assert held[0].robust_scores()["kernel_center"] and held[0].robust_scores()["section_z"]["sec"]
    # the dict-input path carries them too: they need the table only
    from nvrx_straggler import Statistic as S

    summ = {S.MIN: 1.0, S.MAX: 2.0, S.MED: 1.5, S.AVG: 1.5, S.STD: 0.1, S.NUM: 4}
    t = gen.generate_report({"sec": summ}, {"gemm": summ}).robust_scores()
    assert t["section_center"] == {"sec": 1.5} and t["kernel_center"] == {"gemm": 1.5}


def test_thresholds_are_strict_and_nan_is_never_flagged():
    from nvrx_straggler.reporting import Report

    rep = Report({}, {}, {}, {}, {0: "a", 1: "b", 2: "c"}, {}, {}, 0.0, True, 0)
    rep.__dict__["_robust"] = {"gpu_z": {0: 3.5, 1: 3.6, 2: float("nan")},
                               "section_z": {"s": {0: float("inf"), 1: -9.0, 2: float("nan")}, "t": {0: 1.0, 1: 2.0, 2: 3.5}}}
    found = rep.identify_robust_stragglers()
    assert {s.rank for s in found["straggler_gpus_relative"]} == {1}
    assert {n: {s.rank for s in v} for n, v in found["straggler_sections_relative"].items()} == {"s": {0}}
    found = rep.identify_robust_stragglers(gpu_z_threshold=10.0, section_z_threshold=0.5)
    assert found["straggler_gpus_relative"] == set()
    assert {n: {s.rank for s in v} for n, v in found["straggler_sections_relative"].items()} == {"s": {0}, "t": {0, 1, 2}}


# ---- 8. the lane declines ---------------------------------------------------------------------------------------------------
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
                                   _direct=None, asynchronous=False, kernel_attribution=0, tail_q_ppm=0, robust_scores=on)
        rings = SimpleNamespace(lib=SimpleNamespace(nvrx_window_report=object()))
        return SimpleNamespace(_rings=rings, reporter=reporter, _cupti_manager=Manager(), _pending_region_switch=None)

    with pytest.raises(Reached):
        straggler._Lane.build(det(False))
    assert straggler._Lane.build(det(True)) is None


# ---- 9. the C entry points check their arguments before any device is touched ------------------------------------------------
def test_entry_points_check_their_arguments_without_a_device():
    import ctypes

    from nvrx_straggler import _native

    lib = _native.load()
    assert {"nvrx_robust_score", "nvrx_report_robust"} <= {name for name, _, _ in _native.SYMBOLS}
    assert lib.nvrx_abi_version() == 2
    assert _native.robust_words(8, 35, 64) == 4 * 99 + 8 * 2 * 65 and _native.ROBUST_MAX_RANKS == 65536
    fake = ctypes.c_void_p(4096)

    def score(table=fake, R=8, K=8, S=2, first=0, n=8, min_ranks=4, floor=0.02, out=fake):
        return lib.nvrx_robust_score(table, R, K, S, first, n, min_ranks, floor, out, None)

    assert score(R=0) == _native.ERR_INVALID and b"shape" in lib.nvrx_last_error()
    assert score(R=-1) == _native.ERR_INVALID and score(K=-1) == _native.ERR_INVALID and score(S=-1) == _native.ERR_INVALID
    assert score(R=65537, n=1) == _native.ERR_RANGE and b"ranks" in lib.nvrx_last_error()
    assert score(K=70000) == _native.ERR_RANGE
    assert score(first=7, n=2) == _native.ERR_RANGE and b"outside the table" in lib.nvrx_last_error()
    assert score(first=-1) == _native.ERR_RANGE and score(n=0) == _native.ERR_RANGE and score(n=9) == _native.ERR_RANGE
    assert score(min_ranks=0) == _native.ERR_RANGE and b"min_ranks" in lib.nvrx_last_error()
    assert score(min_ranks=-3) == _native.ERR_RANGE
    assert score(floor=float("nan")) == _native.ERR_INVALID and b"floor_rel" in lib.nvrx_last_error()
    assert score(floor=float("inf")) == _native.ERR_INVALID
    assert score(floor=-0.5) == _native.ERR_RANGE and score(floor=1.5) == _native.ERR_RANGE
    assert score(table=None) == _native.ERR_INVALID and score(out=None) == _native.ERR_INVALID
    assert b"null" in lib.nvrx_last_error()
    assert score(out=ctypes.c_void_p(4100)) == _native.ERR_INVALID and b"aligned" in lib.nvrx_last_error()

    desc = _native.ReportDesc()
    desc.R, desc.K, desc.S = 8, 8, 2

    def report(ctx=fake, d=ctypes.byref(desc), first=0, n=8, min_ranks=4, floor=0.02, out=fake):
        return lib.nvrx_report_robust(ctx, d, first, n, min_ranks, floor, out)

    assert report(ctx=None) == _native.ERR_INVALID and report(d=None) == _native.ERR_INVALID
    assert report(first=1) == _native.ERR_RANGE and report(n=0) == _native.ERR_RANGE
    assert report(min_ranks=0) == _native.ERR_RANGE and report(floor=float("nan")) == _native.ERR_INVALID
    assert report(floor=2.0) == _native.ERR_RANGE
    assert report(out=None) == _native.ERR_INVALID and report(out=ctypes.c_void_p(4104)) == _native.ERR_INVALID
