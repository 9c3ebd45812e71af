"""Period scores, host side, on the CPU checker backend (tests/period_oracle_backend.py): the definition on the issue's own
example, the option's plumbing through ReportGenerator / Detector / Report, the collectives of the period step on gloo ranks,
the headline case of a rank that stalls on every 50th sample, lifetime and pickling, the argument checks of the C entry
points (callable without a device), and the cap on the rows of the GPU tests' inputs whose period the bounds do not pin down.

Bounds: period records and section period scores are compared exactly (the checker backend IS the NumPy definition; one f64
quotient rounded to f32); GPU period scores within 2e-6 absolute, the project's tolerance for GPU scores.  The headline's
bounds are the ones its scenario implies: a 1.5 x stall scores 1 / 1.5 = 0.667 (within 0.02: the 1 % noise moves the mean of
the 40 slow samples by 1 % / sqrt(40) = 0.16 %), every rank without a beat scores 1 (>= 0.98), and one slow sample in fifty
moves no median (>= 0.99)."""
import copy
import json
import math
import pickle

import numpy as np
import pytest

import period_workers
from mp_util import run_ranks
from period_oracle_backend import (PeriodOracleBackend, SpyPeriodBackend, choose, fold_curves, period_cap, period_excess,
                                   row_period, row_period_one)


@pytest.fixture
def cpu_backend():
    from nvrx_straggler import backend

    be = PeriodOracleBackend()
    backend.set_backend(be)
    try:
        yield be
    finally:
        backend.set_backend(None)


# ---- 1. the definition, the option's values ---------------------------------------------------------------------------------
def test_definition_on_the_beat_noise_and_burst_rows():
    """The issue's own example: 2000 samples, 1 % noise, seed 17.  Rank 3 stalls on every 50th sample: period 50, strength
    0.98, last seen 36 samples ago -- with a median and a 0.95-quantile like everybody's.  Noise alone and 2 % random
    bursts stay an order of magnitude below the 0.5 default."""
    data = period_workers.headline_data()
    beat, burst = period_workers.BEAT_RANK, period_workers.BURST_RANK
    rec, curves, phases, _ = row_period(data[:, 0, :], [2000] * 8, 1024)
    assert (rec["period"][beat], rec["ago"][beat], phases[beat]) == (50, 36, 13)
    assert 0.97 < rec["strength"][beat] < 0.99 and abs(rec["peak"][beat] - 1500.0) < 5.0 and abs(rec["rest"][beat] - 1000.0) < 1.0
    med = np.median(data[:, 0, :], axis=1)
    q95 = np.quantile(data[:, 0, :], 0.95, axis=1)
    assert np.ptp(med) < 2.0 and np.ptp(q95) < 4.0  # (1000 +- 0.5 and 1016 .. 1019: the beat shows in neither)
    for r in range(8):
        if r != beat:
            assert rec["strength"][r] <= 0.07, (r, rec[r])
            assert period_excess(rec["period"][r], rec["peak"][r], rec["rest"][r], rec["strength"][r], 0.5) == 1.0
    assert period_excess(50, rec["peak"][beat], rec["rest"][beat], rec["strength"][beat], 0.5) == np.float32(
        np.float64(rec["peak"][beat]) / np.float64(rec["rest"][beat]))
    # every multiple of the period explains as much; the rule lands on the fundamental, and a divisor explains at most 1 / k
    c = curves[beat]
    assert all(c[P - 2] >= 0.95 * c.max() for P in range(50, 501, 50)) and c[25 - 2] < 0.5 * c.max() + 0.05
    assert len(c) == 2000 // 4 - 1
    # a beat DOWN (a fast sample) is found just as well: the slow phase is then any of the others, and the excess stays small
    down = data[0, 0].copy()
    down[3::10] *= np.float32(0.5)
    (period, ago, peak, rest, strength), _, _ = row_period_one(down, 1024)
    assert period == 10 and strength > 0.9 and period_excess(period, peak, rest, strength, 0.5) < 1.1
    # a row that also stepped: the step dominates SST and the beat reads weak
    both = data[beat, 0].copy()
    both[1400:] *= np.float32(1.5)
    assert row_period_one(both, 1024)[0][4] < 0.1


def test_period_cap_and_the_short_constant_and_non_finite_rows():
    from nvrx_straggler import _native

    assert (_native.PERIOD_PLANES, _native.PERIOD_MIN_CYCLES, _native.PERIOD_MAX) == (7, 4, 4096)
    for n, mp, want in ((7, 1024, 1), (8, 1024, 2), (9, 1024, 2), (2000, 1024, 500), (10000, 1024, 1024), (65536, 64, 64)):
        assert period_cap(n, mp) == want
    for good in (2, 1024, 4096):
        assert _native.period_max(good) == good
    ones = np.ones((1, 64), dtype=np.float32)
    for n, want in ((0, (0, 0, -1.0, -1.0, -1.0)), (1, (0, 0, 1.0, 1.0, 0.0)), (7, (0, 0, 1.0, 1.0, 0.0)), (8, (0, 0, 1.0, 1.0, 0.0)),
                    (64, (0, 0, 1.0, 1.0, 0.0))):
        assert row_period(ones, [n], 1024)[0][0].tolist() == want, n
    ramp7 = np.arange(64, dtype=np.float32)[None, :]
    assert row_period(ramp7, [7], 1024)[0][0].tolist() == (0, 0, 3.0, 3.0, 0.0)  # (too short: the mean)
    bad = ones.copy()
    for v in (np.nan, np.inf):
        bad[0, 5] = v
        rec = row_period(bad, [64], 1024)[0][0]
        assert rec["period"] == 0 and rec["ago"] == 0 and np.isnan([rec["peak"], rec["rest"], rec["strength"]]).all()
    assert period_excess(0, np.nan, np.nan, np.nan, 0.5) == 1.0 and period_excess(0, 2.0, 1.0, 1.0, 0.5) == 1.0
    # ring starts: the same samples rotated give the same record
    rng = np.random.default_rng(1)
    x = rng.normal(10.0, 0.1, 64).astype(np.float32)
    x[2::7] += 5.0
    base = row_period(x[None, :], [64], 1024)[0][0]
    assert base["period"] == 7 and base["ago"] == (63 - 2) % 7
    for start in (1, 3, 32, 63):
        assert row_period(np.roll(x, start)[None, :], [64], 1024, starts=[start])[0][0] == base


def test_option_values(cpu_backend, monkeypatch):
    from nvrx_straggler import Detector
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(["relative_perf_scores"], period_detection=True)
    assert gen.period_max == 1024 and gen.period_min_strength == 0.5
    gen = ReportGenerator(["relative_perf_scores"], period_detection=True, period_max=64, period_min_strength=0.25)
    assert gen.period_max == 64 and gen.period_min_strength == 0.25
    assert ReportGenerator(["relative_perf_scores"]).period_max == 0
    assert ReportGenerator(["individual_perf_scores"], period_max="nonsense").period_max == 0  # (off: not looked at)
    for bad in (0, 1, 4097, -5, 2.5, "x", None, float("nan")):
        with pytest.raises(ValueError, match="period_max"):
            ReportGenerator(["relative_perf_scores"], period_detection=True, period_max=bad)
    for bad in (-0.1, 1.5, "x", None, float("nan")):
        with pytest.raises(ValueError, match="period_min_strength"):
            ReportGenerator(["relative_perf_scores"], period_detection=True, period_min_strength=bad)
    with pytest.raises(ValueError, match="period_detection.*relative_perf_scores"):
        ReportGenerator(["individual_perf_scores"], period_detection=True)
    with pytest.raises(ValueError, match="period_detection.*relative_perf_scores"):
        Detector.initialize(scores_to_compute=["individual_perf_scores"], period_detection=True)
    assert not Detector.initialized
    # the environment variable is the Detector's default, read only when the argument is None
    monkeypatch.setenv("NVRX_PERIOD_DETECTION", "1")
    Detector.initialize(node_name="n0")
    try:
        assert Detector.reporter.period_max == 1024 and Detector.reporter.onset_seg_ppm == 0
    finally:
        Detector.shutdown()
    Detector.initialize(node_name="n0", period_detection=False)
    try:
        assert Detector.reporter.period_max == 0
    finally:
        Detector.shutdown()
    monkeypatch.setenv("NVRX_PERIOD_DETECTION", "0")
    Detector.initialize(node_name="n0")
    try:
        assert Detector.reporter.period_max == 0
    finally:
        Detector.shutdown()
    monkeypatch.delenv("NVRX_PERIOD_DETECTION")
    Detector.initialize(node_name="n0", period_detection=True, period_max=200, period_min_strength=0.9)
    try:
        assert Detector.reporter.period_max == 200 and Detector.reporter.period_min_strength == 0.9
    finally:
        Detector.shutdown()
    Detector.initialize(node_name="n0")
    try:
        assert Detector.reporter.period_max == 0
    finally:
        Detector.shutdown()


def test_option_needs_a_backend_with_period_score():
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator
    from onset_oracle_backend import OnsetOracleBackend

    backend.set_backend(OnsetOracleBackend())
    try:
        with pytest.raises(RuntimeError, match="no period scores"):
            ReportGenerator(["relative_perf_scores"], period_detection=True)
        ReportGenerator(["relative_perf_scores"], period_detection=False, onset_detection=True)
    finally:
        backend.set_backend(None)


# ---- 2. off by default: nothing is called -----------------------------------------------------------------------------------
@pytest.mark.parametrize("emulate_fused,asynchronous", [(False, False), (True, False), (True, True)])
def test_default_is_off_and_calls_nothing(emulate_fused, asynchronous):
    from nvrx_straggler import Detector
    from nvrx_straggler import Statistic as S
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator

    be = SpyPeriodBackend(emulate_fused=emulate_fused)
    backend.set_backend(be)
    try:
        gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=True, node_name="n",
                              asynchronous=asynchronous)
        assert gen.period_max == 0
        summ = {S.MIN: 1.0, S.MAX: 2.0, S.MED: 1.5, S.AVG: 1.5, S.STD: 0.1, S.NUM: 4}
        rep = gen.generate_report({"sec": summ}, {"k": summ})
        assert rep.period_scores() == {} and pickle.loads(pickle.dumps(rep)).period_scores() == {}
        assert rep.identify_period_stragglers() == {"straggler_gpus_relative": set(), "straggler_sections_relative": {}}
        rings = be.make_rings(1, 8, 32)
        krow, srow = rings.row_for(1, "kern"), rings.row_for(0, "sec")
        kernel_rows, section_rows = {"kern": krow}, {"sec": srow}
        for i in range(3):
            rings.push_many(krow, np.arange(20) + i)
            rings.push_many(srow, np.arange(40))  # (wraps the 32-deep ring)
            rep = gen.generate_report_from_rings(rings, section_rows, kernel_rows)
            rings.reset()
            assert rep.period_scores() == {}
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
                assert rep.period_scores() == {}
                assert set(rep.section_relative_perf_scores) == {"a", "b"}
        finally:
            Detector.shutdown()
        assert be.period_calls == 0
    finally:
        backend.set_backend(None)


# ---- 3. the period step's collectives on gloo ranks ---------------------------------------------------------------------------
def _expected_periods(res, world, i):
    """name -> {rank: record dict} of report i from what every rank pushed (collective kernels are not exchanged)."""
    exp = {}
    for r in range(world):
        for key, vals in res[r]["reports"][i]["pushed"].items():
            if "ncclDev" in key:
                continue
            v = np.array(vals, dtype=np.float32)
            (period, ago, peak, rest, strength), _, _ = row_period_one(v, 1024)
            exp.setdefault(key, {})[r] = {"period": int(period), "samples_ago": int(ago), "peak": float(peak), "rest": float(rest),
                                          "excess": float(period_excess(period, peak, rest, strength, 0.5)),
                                          "strength": float(strength), "window": v.size}
    return exp


@pytest.mark.parametrize("world,gather_on_rank0,tail_quantile,onset_detection",
                         [(2, True, 0.0, False), (2, False, 0.0, False), (3, True, 0.9, True), (3, False, 0.0, True)])
def test_every_rank_issues_the_same_collectives_and_periods_are_right(world, gather_on_rank0, tail_quantile, onset_detection):
    """Every rank issues the period step's all-gather at every report: when new names appear (reports 3 and 5), when a planned
    report fell back, on ranks that hold no report.  With tails and onsets on as well the three steps run one after the
    other, each with its own all-gather; the period rows travel last."""
    res = run_ranks(period_workers.ring_reports_recorded, world, timeout=300, gather_on_rank0=gather_on_rank0,
                    tail_quantile=tail_quantile, onset_detection=onset_detection)
    follow_ups = 1 + bool(tail_quantile) + bool(onset_detection)
    for i in range(6):
        seqs = [res[r]["calls"][i] for r in range(world)]
        assert all(s == seqs[0] for s in seqs), (i, seqs)  # the same collectives on every rank, whatever its report found
        rows = [c[1] for c in seqs[0] if c[0] == "rows"]
        assert len(rows) >= 1 + follow_ups and rows[-1] % 7 == 0, (i, seqs[0])
        KS = rows[-1] // 7
        if onset_detection:
            assert rows[-2] == 6 * KS, (i, seqs[0])
        if tail_quantile:
            assert rows[-3] == KS and rows[-3] < rows[-4], (i, seqs[0])
    assert all(res[r]["period_local_calls"] == 6 and res[r]["onset_enable_calls"] == 1 for r in range(world))
    assert all(res[r]["onset_local_calls"] == (6 if onset_detection else 0) for r in range(world))
    for r in range(world):
        assert res[r]["period_score_calls"] == (6 if (r == 0 or not gather_on_rank0) else 0)
    shapes = set()
    found_beat = 0
    for i in range(6):
        exp = _expected_periods(res, world, i)
        for r in range(world):
            entry = res[r]["reports"][i]
            if gather_on_rank0 and r != 0:
                assert entry["periods"] is None
                continue
            t = entry["periods"]
            assert entry["pickled_same"] and t["max_period"] == 1024 and t["min_strength"] == 0.5
            assert bool(entry["tails"]) == bool(tail_quantile) and bool(entry["onsets"]) == bool(onset_detection)
            shapes.add(tuple(sorted(t)))
            covered = list(range(world)) if gather_on_rank0 else [r]
            assert sorted(t["gpu_relative"]) == covered
            for kind, got in (("section", t["section_periods"]), ("kernel", t["kernel_periods"])):
                want = {k.split(":", 1)[1]: {rr: v for rr, v in per.items() if rr in covered}
                        for k, per in exp.items() if k.startswith(kind)}
                want = {k: v for k, v in want.items() if v}
                assert got == want, (i, r, kind, got, want)
            # section period scores: the steadiest rank's excess over this rank's, NaN where some rank lacks the section
            for name, per in t["section_relative"].items():
                ex = {rr: v["excess"] for rr, v in exp.get(f"section:{name}", {}).items()}
                for rr, score in per.items():
                    if len(ex) < world or rr not in ex:
                        assert math.isnan(score), (i, r, name, rr, score)
                    else:
                        ref = np.float32(min(ex.values()))
                        assert score == float(np.float32(np.float64(ref) / np.float64(np.float32(ex[rr])))), (i, name, rr)
            want_flags = {}
            for name in t["section_relative"]:
                ex = {rr: v["excess"] for rr, v in exp.get(f"section:{name}", {}).items()}
                low = sorted(rr for rr in covered if len(ex) == world and min(ex.values()) / ex[rr] < 0.75)
                if low:
                    want_flags[name] = low
            assert entry["flagged"] == want_flags, (i, entry["flagged"], want_flags)
            # rank 1's s0 stalls on every 3rd sample: found once the window holds four repetitions, and rank 1 alone is flagged
            s0 = exp["section:s0"]
            if 1 in covered and s0[1]["window"] >= 24:
                n = s0[1]["window"]
                assert s0[1]["period"] == 3 and s0[1]["samples_ago"] == (n - 2) % 3 and abs(s0[1]["excess"] - 1.5) < 0.02, (i, s0[1])
                assert entry["flagged"] == {"s0": [1]}, (i, entry["flagged"])
                found_beat += 1
            for rr in covered:  # GPU period score: kernels every rank has (k0: no beat that clears 0.5)
                assert abs(t["gpu_relative"][rr] - 1.0) <= 2e-6, (i, rr, t["gpu_relative"][rr])
    assert found_beat >= 3
    assert shapes == {("gpu_relative", "kernel_periods", "max_period", "min_strength", "section_periods", "section_relative")}


def test_result_shapes_are_the_same_with_and_without_gather_on_rank0():
    on = run_ranks(period_workers.ring_reports_recorded, 2, timeout=300, gather_on_rank0=True)
    off = run_ranks(period_workers.ring_reports_recorded, 2, timeout=300, gather_on_rank0=False)
    for i in range(6):
        whole = on[0]["reports"][i]["periods"]
        for r in range(2):
            part = off[r]["reports"][i]["periods"]
            assert sorted(part) == sorted(whole)
            assert part["gpu_relative"] == {r: whole["gpu_relative"][r]} or all(
                math.isnan(v) for v in (part["gpu_relative"][r], whole["gpu_relative"][r]))
            for key in ("section_periods", "kernel_periods"):
                assert part[key] == {n: {r: per[r]} for n, per in whole[key].items() if r in per}, (i, r, key)
            assert set(part["section_relative"]) <= set(whole["section_relative"])
            assert set(part["section_relative"]) >= set(part["section_periods"])
            for n, per in part["section_relative"].items():
                a, b = per[r], whole["section_relative"][n][r]
                assert a == b or (math.isnan(a) and math.isnan(b)), (i, r, n)


# ---- 4. the headline case -----------------------------------------------------------------------------------------------------
def check_headline(s, data, exact=True):
    """``s``: ``period_workers.summarise`` of a report covering all 8 ranks."""
    R, S, N = period_workers.RANKS, period_workers.SECTIONS, period_workers.SAMPLES
    names = [f"section_{i:03d}" for i in range(S)]
    beat, burst = period_workers.BEAT_RANK, period_workers.BURST_RANK
    assert s["median_flagged"] == [], s["median_flagged"]  # identify_stragglers() names nobody
    assert s["onset_flagged"] == [], s["onset_flagged"]    # ... and neither does identify_onset_stragglers()
    for n in names:
        assert min(s["section_relative"][n].values()) >= 0.99, (n, s["section_relative"][n])  # medians: nobody is slow
    t = s["periods"]
    assert s["period_gpus"] == []  # (no kernels: the GPU period score is NaN)
    assert all(math.isnan(v) for v in t["gpu_relative"].values()) and t["kernel_periods"] == {}
    assert sorted(s["period_sections"]) == names and all(v == [beat] for v in s["period_sections"].values())
    for i, n in enumerate(names):
        for r in range(R):
            rec = t["section_periods"][n][r]
            score = t["section_relative"][n][r]
            assert rec["window"] == N
            if r == beat:
                assert rec["period"] == period_workers.BEAT and rec["samples_ago"] == 36, (n, rec)
                assert abs(rec["excess"] - 1.5) <= 0.02 and abs(score - 1.0 / 1.5) <= 0.02, (n, rec, score)
                assert rec["strength"] > 0.95
            else:
                assert score >= 0.98 and rec["excess"] == 1.0, (n, r, score, rec)
                assert rec["strength"] < 0.5, (n, r, rec)
            if exact:
                (period, ago, peak, rest, strength), _, _ = row_period_one(data[r, i], 1024)
                assert rec == {"period": int(period), "samples_ago": int(ago), "peak": float(peak), "rest": float(rest),
                               "excess": float(period_excess(period, peak, rest, strength, 0.5)), "strength": float(strength),
                               "window": N}, (n, r)


def _report_of(cpu_backend, data, **options):
    from nvrx_straggler.reporting import ReportGenerator

    R, S, N = data.shape
    gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=True, node_name="n", period_detection=True, **options)
    rings = cpu_backend.make_rings(R, S, N)
    names = [f"section_{s:03d}" for s in range(S)]
    rows = {n: rings.row_for(0, n) for n in names}
    for lr in range(R):
        for s, n in enumerate(names):
            rings.samples[lr * S + rows[n]] = data[lr, s]
    rings.total[:] = N
    return gen.generate_report_from_rings(rings, rows, {}, local_ranks=R)


def test_rank_that_stalls_on_a_beat_is_invisible_to_medians_and_onsets_and_flagged_by_periods(cpu_backend):
    data = period_workers.headline_data()
    rep = _report_of(cpu_backend, data, onset_detection=True)
    s = period_workers.summarise(rep)
    assert s["onsets"]  # (the onset scores were there to name somebody)
    check_headline(s, data)


def test_a_beat_of_the_whole_job_flags_nobody(cpu_backend):
    data = period_workers.jobwide_data()
    s = period_workers.summarise(_report_of(cpu_backend, data))
    assert s["period_sections"] == {} and s["period_gpus"] == [] and s["median_flagged"] == []
    t = s["periods"]
    for n, per in t["section_periods"].items():
        for r, rec in per.items():
            assert rec["period"] == period_workers.JOB_BEAT and abs(rec["excess"] - 1.5) <= 0.02, (n, r, rec)
            assert rec["samples_ago"] == (period_workers.SAMPLES - 1 - period_workers.JOB_PHASE) % period_workers.JOB_BEAT
            assert t["section_relative"][n][r] >= 0.98, (n, r, t["section_relative"][n][r])


# ---- 5. lifetime and pickling -------------------------------------------------------------------------------------------------
def test_a_held_report_keeps_its_periods_and_reports_travel(cpu_backend):
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=True, node_name="n",
                          period_detection=True, onset_detection=True, tail_quantile=0.9)
    rings = cpu_backend.make_rings(1, 8, 32)
    kernel_rows = {n: rings.row_for(1, n) for n in ("gemm", "ncclDevKernel_y")}
    section_rows = {"sec": rings.row_for(0, "sec")}
    held = []
    for w in range(4):
        v = np.full(24, 2.0 + w, dtype=np.float32)
        v[w % 3::3] *= np.float32(2.0)  # every 3rd sample, from phase w % 3
        rings.push_many(kernel_rows["gemm"], v)
        rings.push_many(kernel_rows["ncclDevKernel_y"], v * 100)
        rings.push_many(section_rows["sec"], v + 0.5)
        held.append(gen.generate_report_from_rings(rings, section_rows, kernel_rows))
        rings.reset()
    assert gen._ring_plan is not None and cpu_backend.period_score_calls == 4 and cpu_backend.onset_enable_calls == 1
    assert all(h.reads == 0 for h in cpu_backend.period_handles)  # generate_report reads nothing
    for w in (3, 2, 1, 0):
        t = held[w].period_scores()
        assert cpu_backend.period_handles[w].reads == 1
        assert t["kernel_periods"] == {"gemm": {0: {"period": 3, "samples_ago": (23 - w % 3) % 3, "peak": 2.0 * (2.0 + w),
                                                    "rest": 2.0 + w, "excess": 2.0, "strength": 1.0, "window": 24}}}
        assert t["section_periods"]["sec"][0]["period"] == 3 and t["section_periods"]["sec"][0]["strength"] == 1.0
        assert t["gpu_relative"] == {0: 1.0} and t["section_relative"] == {"sec": {0: 1.0}}  # one rank is its own reference
        assert held[w].period_scores() == t and cpu_backend.period_handles[w].reads == 1
        assert held[w].onset_scores() and held[w].tail_scores()
        for clone in (pickle.loads(pickle.dumps(held[w])), copy.deepcopy(held[w])):
            assert json.dumps(clone.period_scores()) == json.dumps(t)
            assert clone.identify_period_stragglers() == held[w].identify_period_stragglers()
    t = held[0].period_scores()
    t["kernel_periods"]["gemm"][0].clear()
    t["section_relative"]["sec"].clear()
    assert held[0].period_scores()["kernel_periods"]["gemm"][0] and held[0].period_scores()["section_relative"]["sec"]
    # the dict-input path has no samples: no periods
    from nvrx_straggler import Statistic as S

    summ = {S.MIN: 1.0, S.MAX: 2.0, S.MED: 1.5, S.AVG: 1.5, S.STD: 0.1, S.NUM: 4}
    assert gen.generate_report({"sec": summ}, {"gemm": summ}).period_scores() == {}


def test_a_wrapped_ring_is_walked_in_time_order(cpu_backend):
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=True, node_name="n", period_detection=True)
    rings = cpu_backend.make_rings(1, 4, 64)
    rows = {"sec": rings.row_for(0, "sec")}
    v = np.full(96, 3.0, dtype=np.float32)
    v[4::5] = 6.0  # the surviving window is v[32:]: its slow samples sit at 2, 7, ... of the window, the last one at 62
    rings.push_many(rows["sec"], v)
    rec = gen.generate_report_from_rings(rings, rows, {}).period_scores()["section_periods"]["sec"][0]
    assert rec == {"period": 5, "samples_ago": 1, "peak": 6.0, "rest": 3.0, "excess": 2.0, "strength": 1.0, "window": 64}


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

    def det(period_max):
        reporter = SimpleNamespace(_ring_plan=SimpleNamespace(fused=True, ws=None), world_size=1, _exchanged=lambda: True,
                                   _direct=None, asynchronous=False, kernel_attribution=0, tail_q_ppm=0, onset_seg_ppm=0,
                                   period_max=period_max)
        rings = SimpleNamespace(lib=SimpleNamespace(nvrx_window_report=object()))
        return SimpleNamespace(_rings=rings, reporter=reporter, _cupti_manager=Manager(), _pending_region_switch=None)

    with pytest.raises(Reached):
        straggler._Lane.build(det(0))
    assert straggler._Lane.build(det(1024)) is None


# ---- 7. the C entry points check their arguments before any device is touched ------------------------------------------------
def test_entry_points_check_their_arguments_without_a_device():
    import ctypes

    from nvrx_straggler import _native

    lib = _native.load()
    assert {"nvrx_row_period", "nvrx_period_score", "nvrx_period_local"} <= {name for name, _, _ in _native.SYMBOLS}
    assert lib.nvrx_abi_version() == 2
    fake = ctypes.c_void_p(4096)

    def period(samples=fake, counts=fake, starts=None, rows=4, stride=1024, max_period=1024, out=fake):
        return lib.nvrx_row_period(samples, counts, starts, rows, stride, max_period, out, None)

    for mp in (-1, 0, 1, 4097, 1 << 30):
        assert period(max_period=mp) == _native.ERR_RANGE and b"max_period" in lib.nvrx_last_error()
    assert period(rows=-1) == _native.ERR_INVALID and b"rows" in lib.nvrx_last_error()
    assert period(stride=0) == _native.ERR_INVALID and period(stride=1022) == _native.ERR_INVALID
    assert b"row_stride" in lib.nvrx_last_error()
    assert period(stride=65540) == _native.ERR_RANGE
    assert period(samples=None) == _native.ERR_INVALID and period(counts=None) == _native.ERR_INVALID
    assert period(out=None) == _native.ERR_INVALID and b"null" in lib.nvrx_last_error()
    assert period(samples=ctypes.c_void_p(4100)) == _native.ERR_INVALID and b"aligned" in lib.nvrx_last_error()
    assert period(out=ctypes.c_void_p(4104)) == _native.ERR_INVALID and b"aligned" in lib.nvrx_last_error()
    assert period(rows=0) == 0  # nothing to do, nothing touched

    def score(periods=fake, table=fake, R=4, K=8, S=2, first=0, n=4, scratch=fake, out=fake):
        return lib.nvrx_period_score(periods, table, R, K, S, first, n, scratch, out, None)

    assert score(R=0) == _native.ERR_INVALID and b"shape" in lib.nvrx_last_error()
    assert score(R=-1) == _native.ERR_INVALID and score(K=-1) == _native.ERR_INVALID and score(S=-1) == _native.ERR_INVALID
    assert score(K=70000) == _native.ERR_RANGE
    assert score(first=3, n=2) == _native.ERR_RANGE and b"outside the table" in lib.nvrx_last_error()
    assert score(first=-1) == _native.ERR_RANGE and score(n=0) == _native.ERR_RANGE and score(n=5) == _native.ERR_RANGE
    assert score(periods=None) == _native.ERR_INVALID and score(table=None) == _native.ERR_INVALID
    assert score(out=None) == _native.ERR_INVALID
    assert score(scratch=None) == _native.ERR_INVALID and b"scratch" in lib.nvrx_last_error()

    desc = _native.ReportDesc()

    def local(ctx=fake, d=None, max_period=1024, strength=0.5, send=fake, K=8, S=2, rows_active=0):
        return lib.nvrx_period_local(ctx, d, max_period, strength, send, K, S, rows_active, None)

    assert local(ctx=None) == _native.ERR_INVALID and local(send=None) == _native.ERR_INVALID
    assert b"null" in lib.nvrx_last_error()
    assert local(K=-1) == _native.ERR_INVALID and local(S=-1) == _native.ERR_INVALID
    assert local(K=70000) == _native.ERR_RANGE
    for mp in (1, 4097):
        assert local(max_period=mp) == _native.ERR_RANGE and b"max_period" in lib.nvrx_last_error()
        assert local(max_period=mp, d=ctypes.byref(desc)) == _native.ERR_RANGE
    for strength in (-0.5, 1.5, float("nan")):
        assert local(strength=strength) == _native.ERR_RANGE and b"min_strength" in lib.nvrx_last_error()


# ---- 8. the inputs of the GPU tests: the bounds pin down the period of (nearly) every row -------------------------------------
def _cap_check(curves, planted, records, tag):
    band = period_workers.band_rows(curves)
    assert len(band) <= 0.02 * len(curves), (tag, band)
    for r, P in enumerate(planted):  # the oracle itself finds every planted period
        if P:
            assert records["period"][r] == P, (tag, r, P, records[r])


@pytest.mark.parametrize("stride", period_workers.STRIDES)
def test_gpu_inputs_stay_within_the_cap_on_undecided_rows(stride):
    """No more than 2 % of a case's rows may have a candidate period within 1e-9 of the bar 0.95 * a_max (or an a_max within
    1e-9 of 0): there the GPU tests do not compare the period.  The oracle alone says which rows those are."""
    samples, counts, max_period, planted = period_workers.kernel_case(stride)
    rec, curves, _, _ = row_period(samples, counts, max_period)
    _cap_check(curves, planted, rec, ("stride", stride))
    if stride in (64, 1000, 4100, period_workers.LDS_SAMPLES + 4):
        samples, counts, starts, max_period, planted = period_workers.rotation_case(stride)
        rec, curves, _, _ = row_period(samples, counts, max_period, starts)
        _cap_check(curves, planted, rec, ("starts", stride))


@pytest.mark.parametrize("rows,stride", [(1, 10000), (512, 1000), (4096, 256)])
def test_gpu_launch_inputs_stay_within_the_cap_on_undecided_rows(rows, stride):
    samples, counts, max_period, planted = period_workers.launch_case(rows, stride)
    rec, curves, _, _ = row_period(samples, counts, max_period)
    _cap_check(curves, planted, rec, ("launch", rows, stride))
