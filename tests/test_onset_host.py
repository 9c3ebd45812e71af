"""Onset scores, host side, on the CPU checker backend (tests/onset_oracle_backend.py): the definition on the issue's own
example, the option's plumbing through ReportGenerator / Detector / Report, the collectives of the onset step on gloo ranks,
the headline case of a rank that becomes slow part of the way through a window, lifetime and pickling, and the argument
checks of the C entry points (callable without a device).

Bounds: onset records and section onset scores are compared exactly (the checker backend IS the NumPy definition; one f64
quotient rounded to f32); GPU onset scores within 2e-6 absolute, the project's tolerance for GPU scores.  The headline's
bounds are the ones its scenario implies: a 1.5 x step scores 1 / 1.5 = 0.667 (within 0.02: the 1 % noise moves the two
means by 1000 * 0.01 / sqrt(600) = 0.04 %), every rank without a step scores 1 (>= 0.99), and the medians of a row that is
slow on less than half of its samples stay within the noise (>= 0.99)."""
import copy
import json
import math
import pickle

import numpy as np
import pytest

import onset_workers
from mp_util import run_ranks
from onset_oracle_backend import OnsetOracleBackend, SpyOnsetBackend, min_segment, onset_shift, row_onset, row_onset_one


@pytest.fixture
def cpu_backend():
    from nvrx_straggler import backend

    be = OnsetOracleBackend()
    backend.set_backend(be)
    try:
        yield be
    finally:
        backend.set_backend(None)


# ---- 1. the definition, the option's values ---------------------------------------------------------------------------------
def test_definition_on_the_step_noise_and_burst_rows():
    """10 000 samples, 1 % noise: a 1.5 x step at 7000 is found at exactly 7000 with strength 0.997 and leaves the median
    alone; noise alone and 10 % random 1.5 x bursts stay two orders of magnitude below the 0.5 default."""
    rng = np.random.default_rng(0)
    noise = (1000.0 * (1.0 + 0.01 * rng.standard_normal(10000))).astype(np.float32)
    step = noise.copy()
    step[7000:] *= np.float32(1.5)
    bursts = np.where(rng.random(10000) < 0.10, noise * np.float32(1.5), noise).astype(np.float32)
    rec, curves = row_onset(np.stack([noise, step, bursts]), [10000] * 3, 50000)
    assert rec["ago"][1] == 3000 and abs(rec["before"][1] - 1000.0) < 1.0 and abs(rec["after"][1] - 1500.0) < 1.5
    assert 0.99 < rec["strength"][1] <= 1.0
    assert abs(np.median(step) - np.median(noise)) < 0.01 * np.median(noise)
    assert rec["strength"][0] < 0.01 and rec["strength"][2] < 0.01
    assert onset_shift(rec["before"][1], rec["after"][1], rec["strength"][1], 0.5) == np.float32(
        np.float64(rec["after"][1]) / np.float64(rec["before"][1]))
    assert onset_shift(rec["before"][2], rec["after"][2], rec["strength"][2], 0.5) == 1.0
    assert all(len(c) == 10000 - 2 * 500 + 1 for c in curves)
    # a step DOWN is found just as well and is no slow-down: it does not shift
    down = noise.copy()
    down[2000:] *= np.float32(0.5)
    (ago, before, after, strength), _ = row_onset_one(down, 50000)
    assert ago == 8000 and strength > 0.99 and onset_shift(before, after, strength, 0.5) == 1.0


def test_minimum_segment_and_the_short_constant_and_non_finite_rows():
    from nvrx_straggler import _native

    for ppm in (1, 50000, 123457, 500000):
        assert _native.onset_seg_ppm(ppm / 1e6) == ppm
        for n in (1, 15, 16, 17, 160, 161, 2000, 10000, 65536):
            assert _native.onset_min_segment(ppm, n) == min_segment(ppm, n) == max(8, math.ceil(ppm * n / 10**6))
    ones = np.ones((1, 64), dtype=np.float32)
    for n, want in ((0, (0, -1.0, -1.0, -1.0)), (1, (0, 1.0, 1.0, 0.0)), (15, (0, 1.0, 1.0, 0.0)), (16, (8, 1.0, 1.0, 0.0)),
                    (64, (56, 1.0, 1.0, 0.0))):
        assert row_onset(ones, [n], 50000)[0][0].tolist() == want, n
    bad = ones.copy()
    bad[0, 5] = np.nan
    rec = row_onset(bad, [64], 50000)[0][0]
    assert rec["ago"] == 0 and np.isnan([rec["before"], rec["after"], rec["strength"]]).all()
    bad[0, 5] = np.inf
    rec = row_onset(bad, [64], 50000)[0][0]
    assert rec["ago"] == 0 and np.isnan([rec["before"], rec["after"], rec["strength"]]).all()
    assert onset_shift(np.nan, np.nan, np.nan, 0.5) == 1.0
    # ring starts: the same samples rotated give the same record
    rng = np.random.default_rng(1)
    x = rng.normal(10.0, 0.1, 64).astype(np.float32)
    x[40:] += 5.0
    base = row_onset(x[None, :], [64], 50000)[0][0]
    for start in (1, 3, 32, 63):
        assert row_onset(np.roll(x, start)[None, :], [64], 50000, starts=[start])[0][0] == base


def test_option_values(cpu_backend, monkeypatch):
    from nvrx_straggler import Detector
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(["relative_perf_scores"], onset_detection=True)
    assert gen.onset_seg_ppm == 50000 and gen.onset_min_strength == 0.5
    gen = ReportGenerator(["relative_perf_scores"], onset_detection=True, onset_min_segment=0.1, onset_min_strength=0.25)
    assert gen.onset_seg_ppm == 100000 and gen.onset_min_strength == 0.25
    assert ReportGenerator(["relative_perf_scores"]).onset_seg_ppm == 0
    assert ReportGenerator(["individual_perf_scores"], onset_min_segment="nonsense").onset_seg_ppm == 0  # (off: not looked at)
    for bad in (0.0, 0.6, -0.1, "x", None, float("nan")):
        with pytest.raises(ValueError, match="onset_min_segment"):
            ReportGenerator(["relative_perf_scores"], onset_detection=True, onset_min_segment=bad)
    for bad in (-0.1, 1.5, "x", None, float("nan")):
        with pytest.raises(ValueError, match="onset_min_strength"):
            ReportGenerator(["relative_perf_scores"], onset_detection=True, onset_min_strength=bad)
    with pytest.raises(ValueError, match="onset_detection.*relative_perf_scores"):
        ReportGenerator(["individual_perf_scores"], onset_detection=True)
    with pytest.raises(ValueError, match="onset_detection.*relative_perf_scores"):
        Detector.initialize(scores_to_compute=["individual_perf_scores"], onset_detection=True)
    assert not Detector.initialized
    # the environment variable is the Detector's default, read only when the argument is None
    monkeypatch.setenv("NVRX_ONSET_DETECTION", "1")
    Detector.initialize(node_name="n0")
    try:
        assert Detector.reporter.onset_seg_ppm == 50000
    finally:
        Detector.shutdown()
    Detector.initialize(node_name="n0", onset_detection=False)
    try:
        assert Detector.reporter.onset_seg_ppm == 0
    finally:
        Detector.shutdown()
    monkeypatch.setenv("NVRX_ONSET_DETECTION", "0")
    Detector.initialize(node_name="n0")
    try:
        assert Detector.reporter.onset_seg_ppm == 0
    finally:
        Detector.shutdown()
    monkeypatch.delenv("NVRX_ONSET_DETECTION")
    Detector.initialize(node_name="n0", onset_detection=True, onset_min_segment=0.2, onset_min_strength=0.9)
    try:
        assert Detector.reporter.onset_seg_ppm == 200000 and Detector.reporter.onset_min_strength == 0.9
    finally:
        Detector.shutdown()
    Detector.initialize(node_name="n0")
    try:
        assert Detector.reporter.onset_seg_ppm == 0
    finally:
        Detector.shutdown()


def test_option_needs_a_backend_with_onset_score():
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator
    from oracle_backend import OracleBackend

    backend.set_backend(OracleBackend())
    try:
        with pytest.raises(RuntimeError, match="no onset scores"):
            ReportGenerator(["relative_perf_scores"], onset_detection=True)
        ReportGenerator(["relative_perf_scores"], onset_detection=False)
    finally:
        backend.set_backend(None)


# ---- 2. off by default: nothing is called -----------------------------------------------------------------------------------
@pytest.mark.parametrize("emulate_fused,asynchronous", [(False, False), (True, False), (True, True)])
def test_default_is_off_and_calls_nothing(emulate_fused, asynchronous):
    from nvrx_straggler import Detector
    from nvrx_straggler import Statistic as S
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator

    be = SpyOnsetBackend(emulate_fused=emulate_fused)
    backend.set_backend(be)
    try:
        gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=True, node_name="n",
                              asynchronous=asynchronous)
        assert gen.onset_seg_ppm == 0
        summ = {S.MIN: 1.0, S.MAX: 2.0, S.MED: 1.5, S.AVG: 1.5, S.STD: 0.1, S.NUM: 4}
        rep = gen.generate_report({"sec": summ}, {"k": summ})
        assert rep.onset_scores() == {} and pickle.loads(pickle.dumps(rep)).onset_scores() == {}
        assert rep.identify_onset_stragglers() == {"straggler_gpus_relative": set(), "straggler_sections_relative": {}}
        rings = be.make_rings(1, 8, 32)
        krow, srow = rings.row_for(1, "kern"), rings.row_for(0, "sec")
        kernel_rows, section_rows = {"kern": krow}, {"sec": srow}
        for i in range(3):
            rings.push_many(krow, np.arange(20) + i)
            rings.push_many(srow, np.arange(40))  # (wraps the 32-deep ring)
            rep = gen.generate_report_from_rings(rings, section_rows, kernel_rows)
            rings.reset()
            assert rep.onset_scores() == {}
            assert 0 in rep.gpu_individual_perf_scores
        assert gen._ring_plan is not None
        gen.close()
        # ... and through the Detector
        Detector.initialize(scores_to_compute="all", gather_on_rank0=True, node_name="n0", asynchronous=asynchronous)
        try:
            for t in range(3):
                for name, value in (("a", 2.0 + t), ("b", 4.0)):
                    with Detector.detection_section(name, profile_cuda=False):
                        pass
                    sec = Detector.custom_sections[name]
                    sec.cpu_elapsed_times.clear()
                    sec.cpu_elapsed_times.extend(np.full(20, value, dtype=np.float32))
                rep = Detector.generate_report()
                assert rep.onset_scores() == {}
                assert set(rep.section_relative_perf_scores) == {"a", "b"}
        finally:
            Detector.shutdown()
        assert be.onset_calls == 0
    finally:
        backend.set_backend(None)


# ---- 3. the onset step's collectives on gloo ranks ----------------------------------------------------------------------------
def _expected_onsets(res, world, i):
    """name -> {rank: record dict} of report i from what every rank pushed (collective kernels are not exchanged)."""
    exp = {}
    for r in range(world):
        for key, vals in res[r]["reports"][i]["pushed"].items():
            if "ncclDev" in key:
                continue
            v = np.array(vals, dtype=np.float32)
            (ago, before, after, strength), _ = row_onset_one(v, 50000)
            exp.setdefault(key, {})[r] = {"shift": float(onset_shift(before, after, strength, 0.5)), "before": float(before),
                                          "after": float(after), "strength": float(strength), "samples_ago": int(ago),
                                          "window": v.size}
    return exp


@pytest.mark.parametrize("world,gather_on_rank0,tail_quantile", [(2, True, 0.0), (2, False, 0.0), (3, True, 0.9), (3, False, 0.0)])
def test_every_rank_issues_the_same_collectives_and_onsets_are_right(world, gather_on_rank0, tail_quantile):
    """With tails on as well the two steps run one after the other, each with its own all-gather."""
    res = run_ranks(onset_workers.ring_reports_recorded, world, timeout=300, gather_on_rank0=gather_on_rank0,
                    tail_quantile=tail_quantile)
    for i in range(6):
        seqs = [res[r]["calls"][i] for r in range(world)]
        assert all(s == seqs[0] for s in seqs), (i, seqs)  # the same collectives on every rank, whatever its report found
        rows = [c for c in seqs[0] if c[0] == "rows"]
        # the onset rows travel last: six planes of [K+S]; behind the tail rows [K+S] when tails are on
        assert len(rows) >= (3 if tail_quantile else 2) and rows[-1][1] % 6 == 0, (i, seqs[0])
        if tail_quantile:
            assert rows[-1][1] == 6 * rows[-2][1] and rows[-2][1] < rows[-3][1], (i, seqs[0])
    assert all(res[r]["onset_local_calls"] == 6 and res[r]["onset_enable_calls"] == 1 for r in range(world))
    for r in range(world):
        assert res[r]["onset_score_calls"] == (6 if (r == 0 or not gather_on_rank0) else 0)
    shapes = set()
    for i in range(6):
        exp = _expected_onsets(res, world, i)
        for r in range(world):
            entry = res[r]["reports"][i]
            if gather_on_rank0 and r != 0:
                assert entry["onsets"] is None
                continue
            t = entry["onsets"]
            assert entry["pickled_same"] and t["min_segment"] == 0.05 and t["min_strength"] == 0.5
            assert bool(entry["tails"]) == bool(tail_quantile)
            shapes.add(tuple(sorted(t)))
            covered = list(range(world)) if gather_on_rank0 else [r]
            assert sorted(t["gpu_relative"]) == covered
            for kind, got in (("section", t["section_onsets"]), ("kernel", t["kernel_onsets"])):
                want = {k.split(":", 1)[1]: {rr: v for rr, v in per.items() if rr in covered}
                        for k, per in exp.items() if k.startswith(kind)}
                want = {k: v for k, v in want.items() if v}
                assert got == want, (i, r, kind, got, want)
            # section onset scores: the steadiest rank's shift over this rank's, NaN where some rank lacks the section
            for name, per in t["section_relative"].items():
                shifts = {rr: v["shift"] for rr, v in exp.get(f"section:{name}", {}).items()}
                for rr, score in per.items():
                    if len(shifts) < world or rr not in shifts:
                        assert math.isnan(score), (i, r, name, rr, score)
                    else:
                        ref = np.float32(min(shifts.values()))
                        assert score == float(np.float32(np.float64(ref) / np.float64(np.float32(shifts[rr])))), (i, name, rr)
            # flags follow the scores; rank 1's s0 steps up by 1.5 x: found where it is once a third of the window holds the
            # 8-sample segment, and rank 1 alone is flagged for it
            want_flags = {}
            for name in t["section_relative"]:
                shifts = {rr: v["shift"] for rr, v in exp.get(f"section:{name}", {}).items()}
                low = sorted(rr for rr in covered if len(shifts) == world and min(shifts.values()) / shifts[rr] < 0.75)
                if low:
                    want_flags[name] = low
            assert entry["flagged"] == want_flags, (i, entry["flagged"], want_flags)
            s0 = exp["section:s0"]
            if 1 in covered and s0[1]["window"] >= 24:
                n = s0[1]["window"]
                assert s0[1]["samples_ago"] == n - 2 * n // 3 and abs(s0[1]["shift"] - 1.5) < 0.02, (i, s0[1])
                assert entry["flagged"] == {"s0": [1]}, (i, entry["flagged"])
            # GPU onset score: kernels every rank has (k0: nobody shifted)
            for rr in covered:
                assert abs(t["gpu_relative"][rr] - 1.0) <= 2e-6, (i, rr, t["gpu_relative"][rr])
    assert shapes == {("gpu_relative", "kernel_onsets", "min_segment", "min_strength", "section_onsets", "section_relative")}


def test_result_shapes_are_the_same_with_and_without_gather_on_rank0():
    on = run_ranks(onset_workers.ring_reports_recorded, 2, timeout=300, gather_on_rank0=True)
    off = run_ranks(onset_workers.ring_reports_recorded, 2, timeout=300, gather_on_rank0=False)
    for i in range(6):
        whole = on[0]["reports"][i]["onsets"]
        for r in range(2):
            part = off[r]["reports"][i]["onsets"]
            assert sorted(part) == sorted(whole)
            assert part["gpu_relative"] == {r: whole["gpu_relative"][r]} or all(
                math.isnan(v) for v in (part["gpu_relative"][r], whole["gpu_relative"][r]))
            for key in ("section_onsets", "kernel_onsets"):
                assert part[key] == {n: {r: per[r]} for n, per in whole[key].items() if r in per}, (i, r, key)
            # (sections as in the score mappings: a rank's own report shows the sections that rank has)
            assert set(part["section_relative"]) <= set(whole["section_relative"])
            assert set(part["section_relative"]) >= set(part["section_onsets"])
            for n, per in part["section_relative"].items():
                a, b = per[r], whole["section_relative"][n][r]
                assert a == b or (math.isnan(a) and math.isnan(b)), (i, r, n)


# ---- 4. the headline case -----------------------------------------------------------------------------------------------------
def check_headline(s, data, exact=True):
    """``s``: ``onset_workers.summarise`` of a report covering all 8 ranks."""
    R, S, N = onset_workers.RANKS, onset_workers.SECTIONS, onset_workers.SAMPLES
    names = [f"section_{i:03d}" for i in range(S)]
    step, burst = onset_workers.STEP_RANK, onset_workers.BURST_RANK
    assert s["median_flagged"] == [], s["median_flagged"]
    for n in names:
        assert min(s["section_relative"][n].values()) >= 0.99, (n, s["section_relative"][n])  # medians: nobody is slow
    t = s["onsets"]
    assert s["onset_gpus"] == []  # (no kernels: the GPU onset score is NaN)
    assert all(math.isnan(v) for v in t["gpu_relative"].values()) and t["kernel_onsets"] == {}
    assert sorted(s["onset_sections"]) == names and all(v == [step] for v in s["onset_sections"].values())
    for i, n in enumerate(names):
        for r in range(R):
            rec = t["section_onsets"][n][r]
            score = t["section_relative"][n][r]
            assert rec["window"] == N
            if r == step:
                assert abs(score - 1.0 / 1.5) <= 0.02, (n, score)
                assert abs(rec["samples_ago"] - 600) <= 6, (n, rec)
                assert rec["strength"] > 0.99 and abs(rec["shift"] - 1.5) < 0.01
            else:
                assert score >= 0.99 and rec["shift"] == 1.0, (n, r, score, rec)
                if r == burst:
                    assert rec["strength"] < 0.05, (n, rec)
            if exact:
                (ago, before, after, strength), _ = row_onset_one(data[r, i], 50000)
                assert rec == {"shift": float(onset_shift(before, after, strength, 0.5)), "before": float(before),
                               "after": float(after), "strength": float(strength), "samples_ago": int(ago), "window": N}, (n, r)


def test_rank_that_becomes_slow_late_in_the_window_is_invisible_to_medians_and_flagged_by_onsets(cpu_backend):
    from nvrx_straggler.reporting import ReportGenerator

    data = onset_workers.headline_data()
    R, S, N = data.shape
    gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=True, node_name="n", onset_detection=True)
    rings = cpu_backend.make_rings(R, S, N)
    names = [f"section_{s:03d}" for s in range(S)]
    rows = {n: rings.row_for(0, n) for n in names}
    for lr in range(R):
        for s, n in enumerate(names):
            rings.samples[lr * S + rows[n]] = data[lr, s]
    rings.total[:] = N
    rep = gen.generate_report_from_rings(rings, rows, {}, local_ranks=R)
    check_headline(onset_workers.summarise(rep), data)


# ---- 5. lifetime and pickling -------------------------------------------------------------------------------------------------
def test_a_held_report_keeps_its_onsets_and_reports_travel(cpu_backend):
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=True, node_name="n",
                          onset_detection=True, tail_quantile=0.9)
    rings = cpu_backend.make_rings(1, 8, 32)
    kernel_rows = {n: rings.row_for(1, n) for n in ("gemm", "ncclDevKernel_y")}
    section_rows = {"sec": rings.row_for(0, "sec")}
    held = []
    windows = []
    for w in range(4):
        v = np.full(24, 2.0 + w, dtype=np.float32)
        v[10 + w:] *= np.float32(2.0)  # the step sits 14 - w samples before the end
        windows.append(v)
        rings.push_many(kernel_rows["gemm"], v)
        rings.push_many(kernel_rows["ncclDevKernel_y"], v * 100)
        rings.push_many(section_rows["sec"], v + 0.5)
        held.append(gen.generate_report_from_rings(rings, section_rows, kernel_rows))
        rings.reset()
    assert gen._ring_plan is not None and cpu_backend.onset_score_calls == 4 and cpu_backend.onset_enable_calls == 1
    assert all(h.reads == 0 for h in cpu_backend.onset_handles)  # generate_report reads nothing
    for w in (3, 2, 1, 0):
        t = held[w].onset_scores()
        assert cpu_backend.onset_handles[w].reads == 1
        assert t["kernel_onsets"] == {"gemm": {0: {"shift": 2.0, "before": 2.0 + w, "after": 2.0 * (2.0 + w), "strength": 1.0,
                                                   "samples_ago": 14 - w, "window": 24}}}
        assert t["section_onsets"]["sec"][0]["samples_ago"] == 14 - w and t["section_onsets"]["sec"][0]["strength"] == 1.0
        assert t["gpu_relative"] == {0: 1.0} and t["section_relative"] == {"sec": {0: 1.0}}  # one rank is its own reference
        assert held[w].onset_scores() == t and cpu_backend.onset_handles[w].reads == 1
        for clone in (pickle.loads(pickle.dumps(held[w])), copy.deepcopy(held[w])):
            assert json.dumps(clone.onset_scores()) == json.dumps(t)
            assert clone.identify_onset_stragglers() == held[w].identify_onset_stragglers()
    t = held[0].onset_scores()
    t["kernel_onsets"]["gemm"][0].clear()
    t["section_relative"]["sec"].clear()
    assert held[0].onset_scores()["kernel_onsets"]["gemm"][0] and held[0].onset_scores()["section_relative"]["sec"]
    # the dict-input path has no samples: no onsets
    from nvrx_straggler import Statistic as S

    summ = {S.MIN: 1.0, S.MAX: 2.0, S.MED: 1.5, S.AVG: 1.5, S.STD: 0.1, S.NUM: 4}
    assert gen.generate_report({"sec": summ}, {"gemm": summ}).onset_scores() == {}


def test_a_wrapped_ring_is_walked_in_time_order(cpu_backend):
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=True, node_name="n", onset_detection=True)
    rings = cpu_backend.make_rings(1, 4, 64)
    rows = {"sec": rings.row_for(0, "sec")}
    v = np.full(96, 3.0, dtype=np.float32)
    v[80:] = 6.0  # 16 samples before the end; the surviving window is v[32:]
    rings.push_many(rows["sec"], v)
    rec = gen.generate_report_from_rings(rings, rows, {}).onset_scores()["section_onsets"]["sec"][0]
    assert rec == {"shift": 2.0, "before": 3.0, "after": 6.0, "strength": 1.0, "samples_ago": 16, "window": 64}


# ---- 6. the lane declines ---------------------------------------------------------------------------------------------------
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

    def det(seg_ppm):
        reporter = SimpleNamespace(_ring_plan=SimpleNamespace(fused=True, ws=None), world_size=1, _exchanged=lambda: True,
                                   _direct=None, asynchronous=False, kernel_attribution=0, tail_q_ppm=0, onset_seg_ppm=seg_ppm)
        rings = SimpleNamespace(lib=SimpleNamespace(nvrx_window_report=object()))
        return SimpleNamespace(_rings=rings, reporter=reporter, _cupti_manager=Manager(), _pending_region_switch=None)

    with pytest.raises(Reached):
        straggler._Lane.build(det(0))
    assert straggler._Lane.build(det(50000)) is None


# ---- 7. the C entry points check their arguments before any device is touched ------------------------------------------------
def test_entry_points_check_their_arguments_without_a_device():
    import ctypes

    from nvrx_straggler import _native

    lib = _native.load()
    assert {"nvrx_row_onset", "nvrx_onset_score", "nvrx_onset_local", "nvrx_onset_enable"} <= {name for name, _, _ in _native.SYMBOLS}
    assert lib.nvrx_abi_version() == 2
    fake = ctypes.c_void_p(4096)

    def onset(samples=fake, counts=fake, starts=None, rows=4, stride=1024, seg=50000, out=fake):
        return lib.nvrx_row_onset(samples, counts, starts, rows, stride, seg, out, None)

    for seg in (0, 500001, 4000000000):
        assert onset(seg=seg) == _native.ERR_RANGE and b"min_seg_ppm" in lib.nvrx_last_error()
    assert onset(rows=-1) == _native.ERR_INVALID and b"rows" in lib.nvrx_last_error()
    assert onset(stride=0) == _native.ERR_INVALID and onset(stride=1022) == _native.ERR_INVALID
    assert b"row_stride" in lib.nvrx_last_error()
    assert onset(stride=65540) == _native.ERR_RANGE
    assert onset(samples=None) == _native.ERR_INVALID and onset(counts=None) == _native.ERR_INVALID
    assert onset(out=None) == _native.ERR_INVALID and b"null" in lib.nvrx_last_error()
    assert onset(samples=ctypes.c_void_p(4100)) == _native.ERR_INVALID and b"aligned" in lib.nvrx_last_error()
    assert onset(out=ctypes.c_void_p(4104)) == _native.ERR_INVALID and b"aligned" in lib.nvrx_last_error()
    assert onset(rows=0) == 0  # nothing to do, nothing touched

    def score(onsets=fake, table=fake, R=4, K=8, S=2, first=0, n=4, scratch=fake, out=fake):
        return lib.nvrx_onset_score(onsets, table, R, K, S, first, n, scratch, out, None)

    assert score(R=0) == _native.ERR_INVALID and b"shape" in lib.nvrx_last_error()
    assert score(R=-1) == _native.ERR_INVALID and score(K=-1) == _native.ERR_INVALID and score(S=-1) == _native.ERR_INVALID
    assert score(K=70000) == _native.ERR_RANGE
    assert score(first=3, n=2) == _native.ERR_RANGE and b"outside the table" in lib.nvrx_last_error()
    assert score(first=-1) == _native.ERR_RANGE and score(n=0) == _native.ERR_RANGE and score(n=5) == _native.ERR_RANGE
    assert score(onsets=None) == _native.ERR_INVALID and score(table=None) == _native.ERR_INVALID
    assert score(out=None) == _native.ERR_INVALID
    assert score(scratch=None) == _native.ERR_INVALID and b"scratch" in lib.nvrx_last_error()

    desc = _native.ReportDesc()

    def local(ctx=fake, d=None, seg=50000, strength=0.5, send=fake, K=8, S=2, rows_active=0):
        return lib.nvrx_onset_local(ctx, d, seg, strength, send, K, S, rows_active, None)

    assert local(ctx=None) == _native.ERR_INVALID and local(send=None) == _native.ERR_INVALID
    assert b"null" in lib.nvrx_last_error()
    assert local(K=-1) == _native.ERR_INVALID and local(S=-1) == _native.ERR_INVALID
    assert local(K=70000) == _native.ERR_RANGE
    for seg in (0, 500001):
        assert local(seg=seg) == _native.ERR_RANGE and b"min_seg_ppm" in lib.nvrx_last_error()
        assert local(seg=seg, d=ctypes.byref(desc)) == _native.ERR_RANGE
    for strength in (-0.5, 1.5, float("nan")):
        assert local(strength=strength) == _native.ERR_RANGE and b"min_strength" in lib.nvrx_last_error()
    assert lib.nvrx_onset_enable(None, 1) == _native.ERR_INVALID
