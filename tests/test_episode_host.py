"""Episode scores, host side, on the CPU checker backend (tests/episode_oracle_backend.py): the definition on the issue's own
example, the option's plumbing through ReportGenerator / Detector / Report, the collectives of the episode step on gloo ranks,
the headline case of a rank that was slow for one stretch of 60 samples, lifetime and pickling, the argument checks of the C
entry points (callable without a device), and the cap on the rows of the GPU tests' inputs whose interval the bounds do not
pin down.

Bounds: episode records and section episode scores are compared exactly (the checker backend IS the NumPy definition; one f64
quotient rounded to f32); GPU episode scores within 2e-6 absolute, the project's tolerance for GPU scores.  The headline's
bounds are the ones its scenario implies: a 1.5 x stretch scores 1 / 1.5 = 0.667 (within 0.02: the 1 % noise moves the mean of
the 60 slow samples by 1 % / sqrt(60) = 0.13 %), every rank without an episode scores 1 (>= 0.98), and 3 % of a window moves
no median and no 0.95-quantile (>= 0.99)."""
import copy
import json
import math
import pickle

import numpy as np
import pytest

import episode_workers
from episode_oracle_backend import (EpisodeOracleBackend, SpyEpisodeBackend, episode_excess, episode_one, min_len, row_episode)
from mp_util import run_ranks
from onset_oracle_backend import row_onset
from period_oracle_backend import row_period_one


@pytest.fixture
def cpu_backend():
    from nvrx_straggler import backend

    be = EpisodeOracleBackend()
    backend.set_backend(be)
    try:
        yield be
    finally:
        backend.set_backend(None)


def _record(x, len_ppm=5000, min_strength=0.5):
    """The Report's record dict of one row in time order, from the definition."""
    ago, length, inside, outside, strength = episode_one(x, len_ppm).rec
    n = len(x)
    return {"length": int(length), "samples_ago": int(ago), "began_ago": int(ago + length) if length else 0, "window": n,
            "inside": float(inside), "outside": float(outside), "strength": float(strength),
            "excess": float(episode_excess(length, inside, outside, strength, min_strength)),
            "open_ended": bool(length) and int(ago) == min_len(len_ppm, n)}


# ---- 1. the definition, the option's values ---------------------------------------------------------------------------------
def test_definition_on_the_stretch_noise_and_burst_rows():
    """The issue's own example at 2000 samples, 1 % noise, seed 17.  Rank 3 is 1.5 x slower on samples 1200 .. 1259: exactly
    that interval, strength above 0.95 -- with a median and a 0.95-quantile like everybody's, no step and no beat.  Noise
    alone and 2 % random bursts stay an order of magnitude below the 0.5 default."""
    data = episode_workers.headline_data()
    slow, burst = episode_workers.EPISODE_RANK, episode_workers.BURST_RANK
    rec, eps = row_episode(data[:, 0, :], [2000] * 8, 5000)
    assert (eps[slow].a, eps[slow].b) == (episode_workers.BEGIN, episode_workers.END)
    assert (rec["ago"][slow], rec["length"][slow]) == (2000 - episode_workers.END, 60)
    assert rec["strength"][slow] > 0.95 and abs(rec["inside"][slow] - 1500.0) < 5.0 and abs(rec["outside"][slow] - 1000.0) < 1.0
    med = np.median(data[:, 0, :], axis=1)
    q95 = np.quantile(data[:, 0, :], 0.95, axis=1)
    # the stretch shows in neither: medians 1000 +- 0.7; the slow rank's upper 3 % push its 0.95-quantile from the normal
    # 0.95-point (z = 1.64: 1016.4) to the normal part's 0.979-point (z = 2.04: 1020.4), a ratio of 0.996
    assert np.ptp(med) < 2.0 and q95.min() / q95[slow] >= 0.99 and np.ptp(np.delete(q95, slow)) < 4.0
    onset = row_onset(data[:, 0, :], [2000] * 8, 50000)[0]
    assert onset["strength"][slow] < 0.1  # a pulse is no step
    assert row_period_one(data[slow, 0], 1024)[0][4] < 0.1  # ... and no beat
    for r in range(8):
        if r != slow:
            assert rec["strength"][r] <= 0.05, (r, rec[r])
            assert episode_excess(rec["length"][r], rec["inside"][r], rec["outside"][r], rec["strength"][r], 0.5) == 1.0
    assert episode_excess(60, rec["inside"][slow], rec["outside"][slow], rec["strength"][slow], 0.5) == np.float32(
        np.float64(rec["inside"][slow]) / np.float64(rec["outside"][slow]))
    # the README's row: 300 of 10 000
    ep = episode_one(episode_workers.readme_row(), 5000)
    assert (ep.a, ep.b) == (6000, 6300) and ep.rec[4] > 0.95
    # a stretch that is FASTER is found just as well (the rest is then "inside"), and its excess stays 1
    fast = data[0, 0].copy()
    fast[500:900] *= np.float32(0.5)
    ago, length, inside, outside, strength = episode_one(fast, 5000).rec
    assert episode_excess(length, inside, outside, strength, 0.0) < 1.35  # (what is "inside" is the longer normal part)
    # a row on a beat reads as none worth the name
    beat = data[0, 0].copy()
    beat[13::50] *= np.float32(1.5)
    assert episode_one(beat, 5000).rec[4] < 0.1


def test_open_ended_on_a_stepped_row_and_the_ramp():
    """The documented interactions: a row that stepped up reads as a strong episode that runs to the last admissible sample
    (ago == m); a ramp reads as an episode of its upper part."""
    rng = np.random.default_rng(5)
    x = (1000.0 * (1.0 + 0.01 * rng.standard_normal(2000))).astype(np.float32)
    x[1400:] *= np.float32(1.5)
    rec = _record(x)
    m = min_len(5000, 2000)
    assert rec["open_ended"] and rec["samples_ago"] == m == 10 and rec["began_ago"] == 600 and rec["strength"] > 0.9
    assert not _record(episode_workers.headline_data()[episode_workers.EPISODE_RANK, 0])["open_ended"]
    ramp = (1000.0 + 300.0 * np.arange(2000) / 2000 + 10.0 * rng.standard_normal(2000)).astype(np.float32)
    r = _record(ramp)
    assert r["open_ended"] and 0.3 < r["strength"] < 0.8


def test_min_length_and_the_degenerate_rows():
    from nvrx_straggler import _native

    assert (_native.EPISODE_PLANES, _native.EPISODE_MIN_SAMPLES) == (7, 8)
    assert (_native.EPISODE_LEN_PPM_MIN, _native.EPISODE_LEN_PPM_MAX) == (1, 333333)
    for n, ppm, want in ((1, 1, 8), (2000, 1, 8), (65536, 1, 8), (1599, 5000, 8), (1600, 5000, 8), (1601, 5000, 9),
                         (10000, 5000, 50), (65536, 5000, 328), (24, 333333, 8), (25, 333333, 9), (10000, 333333, 3334),
                         (65536, 333333, 21846)):
        assert min_len(ppm, n) == _native.episode_min_samples(ppm, n) == want, (n, ppm)
    for frac, ppm in ((0.005, 5000), (0.000001, 1), (0.333333, 333333), (0.1, 100000)):
        assert _native.episode_len_ppm(frac) == ppm
    ones = np.ones((1, 64), dtype=np.float32)
    for n, want in ((0, (0, 0, -1.0, -1.0, -1.0)), (1, (0, 0, 1.0, 1.0, 0.0)), (23, (0, 0, 1.0, 1.0, 0.0)), (24, (0, 0, 1.0, 1.0, 0.0)),
                    (64, (0, 0, 1.0, 1.0, 0.0))):
        assert row_episode(ones, [n], 5000)[0][0].tolist() == want, n
    ramp = np.arange(64, dtype=np.float32)[None, :]
    assert row_episode(ramp, [23], 5000)[0][0].tolist() == (0, 0, 11.0, 11.0, 0.0)  # (n < 3m: the mean)
    valley = np.concatenate([np.full(10, 5.0), np.full(44, 1.0), np.full(10, 5.0)]).astype(np.float32)[None, :]
    assert row_episode(valley, [64], 5000)[0][0].tolist() == (0, 0, 2.25, 2.25, 0.0)  # (no interval above the mean: the mean)
    bad = ones.copy()
    for v in (np.nan, np.inf):
        bad[0, 5] = v
        rec = row_episode(bad, [64], 5000)[0][0]
        assert rec["length"] == 0 and rec["ago"] == 0 and np.isnan([rec["inside"], rec["outside"], rec["strength"]]).all()
    assert episode_excess(0, np.nan, np.nan, np.nan, 0.5) == 1.0 and episode_excess(0, 2.0, 1.0, 1.0, 0.5) == 1.0
    assert episode_excess(8, 2.0, 1.0, 0.4, 0.5) == 1.0 and episode_excess(8, 2.0, 1.0, 0.5, 0.5) == 2.0
    # the smallest row with a candidate: n = 24, m = 8, the one interval [8, 16)
    x = np.full(24, 2.0, dtype=np.float32)
    x[8:16] = 4.0
    assert row_episode(x[None, :], [24], 1)[0][0].tolist() == (8, 8, 4.0, 2.0, 1.0)
    # ties go to the lowest b, then the lowest a
    x = np.full(64, 2.0, dtype=np.float32)
    x[8:16] = 4.0
    x[48:56] = 4.0  # (a gap of 32 > n / 2 - L = 24 normal samples: the interval spanning both explains less)
    ep = episode_one(x, 1)
    assert (ep.a, ep.b) == (8, 16) and ep.e_at(8, 16) == ep.e_at(48, 56) > ep.e_at(8, 56)
    # ring starts: the same samples rotated give the same record
    rng = np.random.default_rng(1)
    x = rng.normal(10.0, 0.1, 64).astype(np.float32)
    x[20:30] += 5.0
    base = row_episode(x[None, :], [64], 5000)[0][0]
    assert (base["ago"], base["length"]) == (34, 10)
    for start in (1, 3, 32, 63):
        assert row_episode(np.roll(x, start)[None, :], [64], 5000, starts=[start])[0][0] == base


def test_option_values(cpu_backend, monkeypatch):
    from nvrx_straggler import Detector
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(["relative_perf_scores"], episode_detection=True)
    assert gen.episode_len_ppm == 5000 and gen.episode_min_strength == 0.5
    gen = ReportGenerator(["relative_perf_scores"], episode_detection=True, episode_min_length=0.02, episode_min_strength=0.25)
    assert gen.episode_len_ppm == 20000 and gen.episode_min_strength == 0.25
    assert ReportGenerator(["relative_perf_scores"]).episode_len_ppm == 0
    assert ReportGenerator(["individual_perf_scores"], episode_min_length="nonsense").episode_len_ppm == 0  # (off: not looked at)
    for bad in (0, 0.0000001, 0.34, 0.5, 1, -0.01, "x", None, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="episode_min_length"):
            ReportGenerator(["relative_perf_scores"], episode_detection=True, episode_min_length=bad)
    for bad in (-0.1, 1.5, "x", None, float("nan")):
        with pytest.raises(ValueError, match="episode_min_strength"):
            ReportGenerator(["relative_perf_scores"], episode_detection=True, episode_min_strength=bad)
    with pytest.raises(ValueError, match="episode_detection.*relative_perf_scores"):
        ReportGenerator(["individual_perf_scores"], episode_detection=True)
    with pytest.raises(ValueError, match="episode_detection.*relative_perf_scores"):
        Detector.initialize(scores_to_compute=["individual_perf_scores"], episode_detection=True)
    assert not Detector.initialized
    # the environment variable is the Detector's default, read only when the argument is None
    monkeypatch.setenv("NVRX_EPISODE_DETECTION", "1")
    Detector.initialize(node_name="n0")
    try:
        assert Detector.reporter.episode_len_ppm == 5000 and Detector.reporter.onset_seg_ppm == 0 and Detector.reporter.period_max == 0
    finally:
        Detector.shutdown()
    Detector.initialize(node_name="n0", episode_detection=False)
    try:
        assert Detector.reporter.episode_len_ppm == 0
    finally:
        Detector.shutdown()
    monkeypatch.setenv("NVRX_EPISODE_DETECTION", "0")
    Detector.initialize(node_name="n0")
    try:
        assert Detector.reporter.episode_len_ppm == 0
    finally:
        Detector.shutdown()
    monkeypatch.delenv("NVRX_EPISODE_DETECTION")
    Detector.initialize(node_name="n0", episode_detection=True, episode_min_length=0.01, episode_min_strength=0.9)
    try:
        assert Detector.reporter.episode_len_ppm == 10000 and Detector.reporter.episode_min_strength == 0.9
    finally:
        Detector.shutdown()
    Detector.initialize(node_name="n0")
    try:
        assert Detector.reporter.episode_len_ppm == 0
    finally:
        Detector.shutdown()


def test_option_needs_a_backend_with_episode_score():
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator
    from period_oracle_backend import PeriodOracleBackend

    backend.set_backend(PeriodOracleBackend())
    try:
        with pytest.raises(RuntimeError, match="no episode scores"):
            ReportGenerator(["relative_perf_scores"], episode_detection=True)
        ReportGenerator(["relative_perf_scores"], episode_detection=False, period_detection=True)
    finally:
        backend.set_backend(None)


# ---- 2. off by default: nothing is called -----------------------------------------------------------------------------------
@pytest.mark.parametrize("emulate_fused,asynchronous", [(False, False), (False, True), (True, False), (True, True)])
def test_default_is_off_and_calls_nothing(emulate_fused, asynchronous):
    from nvrx_straggler import Detector
    from nvrx_straggler import Statistic as S
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator

    be = SpyEpisodeBackend(emulate_fused=emulate_fused)
    backend.set_backend(be)
    try:
        gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=True, node_name="n",
                              asynchronous=asynchronous)
        assert gen.episode_len_ppm == 0
        summ = {S.MIN: 1.0, S.MAX: 2.0, S.MED: 1.5, S.AVG: 1.5, S.STD: 0.1, S.NUM: 4}
        rep = gen.generate_report({"sec": summ}, {"k": summ})
        assert rep.episode_scores() == {} and pickle.loads(pickle.dumps(rep)).episode_scores() == {}
        assert rep.identify_episode_stragglers() == {"straggler_gpus_relative": set(), "straggler_sections_relative": {}}
        rings = be.make_rings(1, 8, 32)
        krow, srow = rings.row_for(1, "kern"), rings.row_for(0, "sec")
        kernel_rows, section_rows = {"kern": krow}, {"sec": srow}
        for i in range(3):
            rings.push_many(krow, np.arange(20) + i)
            rings.push_many(srow, np.arange(40))  # (wraps the 32-deep ring)
            rep = gen.generate_report_from_rings(rings, section_rows, kernel_rows)
            rings.reset()
            assert rep.episode_scores() == {}
            assert 0 in rep.gpu_individual_perf_scores
            assert "_episode" not in rep.__dict__
        assert gen._ring_plan is not None
        for ws in (gen._ring_plan.ws,):  # no workspace grew an episode buffer
            assert "episode" not in (getattr(ws, "_family_state", None) or {}) and getattr(ws, "_episode_table", None) is None
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
                assert rep.episode_scores() == {}
                assert set(rep.section_relative_perf_scores) == {"a", "b"}
        finally:
            Detector.shutdown()
        assert be.episode_calls == 0
    finally:
        backend.set_backend(None)


# ---- 3. the episode step's collectives on gloo ranks --------------------------------------------------------------------------
def _expected_episodes(res, world, i):
    """name -> {rank: record dict} of report i from what every rank pushed (collective kernels are not exchanged)."""
    exp = {}
    for r in range(world):
        for key, vals in res[r]["reports"][i]["pushed"].items():
            if "ncclDev" in key:
                continue
            exp.setdefault(key, {})[r] = _record(np.array(vals, dtype=np.float32))
    return exp


@pytest.mark.parametrize("world,gather_on_rank0,tail_quantile,onset_detection,period_detection",
                         [(2, True, 0.0, False, False), (2, False, 0.0, False, True), (3, True, 0.9, True, True),
                          (3, False, 0.0, True, False)])
def test_every_rank_issues_the_same_collectives_and_episodes_are_right(world, gather_on_rank0, tail_quantile, onset_detection,
                                                                       period_detection):
    """Every rank issues the episode step's all-gather at every report: when new names appear (reports 3 and 5), when a
    planned report fell back, on ranks that hold no report.  With tails, onsets and periods on as well the four steps run one
    after the other, each with its own all-gather; the episode rows -- 7 (K+S) floats -- travel last."""
    res = run_ranks(episode_workers.ring_reports_recorded, world, timeout=300, gather_on_rank0=gather_on_rank0,
                    tail_quantile=tail_quantile, onset_detection=onset_detection, period_detection=period_detection)
    follow_ups = 1 + bool(tail_quantile) + bool(onset_detection) + bool(period_detection)
    for i in range(6):
        seqs = [res[r]["calls"][i] for r in range(world)]
        assert all(s == seqs[0] for s in seqs), (i, seqs)  # the same collectives on every rank, whatever its report found
        rows = [c[1] for c in seqs[0] if c[0] == "rows"]
        assert len(rows) >= 1 + follow_ups and rows[-1] % 7 == 0, (i, seqs[0])
        KS = rows[-1] // 7
        want = ([KS] if tail_quantile else []) + ([6 * KS] if onset_detection else []) + ([7 * KS] if period_detection else []) + [7 * KS]
        assert rows[-follow_ups:] == want, (i, seqs[0])
        assert rows[-follow_ups - 1] > KS  # (the report's own exchange row: statistics of every id)
    assert all(res[r]["episode_local_calls"] == 6 and res[r]["onset_enable_calls"] == 1 for r in range(world))
    assert all(res[r]["onset_local_calls"] == (6 if onset_detection else 0) for r in range(world))
    assert all(res[r]["period_local_calls"] == (6 if period_detection else 0) for r in range(world))
    for r in range(world):
        assert res[r]["episode_score_calls"] == (6 if (r == 0 or not gather_on_rank0) else 0)
    shapes = set()
    found = 0
    for i in range(6):
        exp = _expected_episodes(res, world, i)
        for r in range(world):
            entry = res[r]["reports"][i]
            if gather_on_rank0 and r != 0:
                assert entry["episodes"] is None
                continue
            t = entry["episodes"]
            assert entry["pickled_same"] and t["min_length"] == 0.005 and t["min_strength"] == 0.5
            assert bool(entry["tails"]) == bool(tail_quantile) and bool(entry["onsets"]) == bool(onset_detection)
            assert bool(entry["periods"]) == bool(period_detection)
            shapes.add(tuple(sorted(t)))
            covered = list(range(world)) if gather_on_rank0 else [r]
            assert sorted(t["gpu_relative"]) == covered and t["gpu_scores"] == t["gpu_relative"]
            assert t["section_scores"] == t["section_relative"] or json.dumps(t["section_scores"]) == json.dumps(t["section_relative"])
            for kind, got in (("section", t["section_episodes"]), ("kernel", t["kernel_episodes"])):
                want = {k.split(":", 1)[1]: {rr: v for rr, v in per.items() if rr in covered}
                        for k, per in exp.items() if k.startswith(kind)}
                want = {k: v for k, v in want.items() if v}
                assert got == want, (i, r, kind, got, want)
            # section episode scores: the steadiest rank's excess over this rank's, NaN where some rank lacks the section
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
            # rank 1's s0 is slow on samples 8 .. 15: found once the window holds 8 normal samples behind them, rank 1 alone
            s0 = exp["section:s0"]
            if 1 in covered and s0[1]["window"] >= 24:
                n = s0[1]["window"]
                assert s0[1]["length"] == 8 and s0[1]["samples_ago"] == n - 16 and abs(s0[1]["excess"] - 1.5) < 0.02, (i, s0[1])
                assert s0[1]["began_ago"] == n - 8
                assert entry["flagged"] == {"s0": [1]}, (i, entry["flagged"])
                found += 1
            for rr in covered:  # GPU episode score: kernels every rank has (k0: no episode that clears 0.5 ... or NaN early on)
                g = t["gpu_relative"][rr]
                assert math.isnan(g) or 0.0 < g <= 1.0 + 2e-6, (i, rr, g)
    assert found >= 3
    assert shapes == {("gpu_relative", "gpu_scores", "kernel_episodes", "min_length", "min_strength", "section_episodes",
                       "section_relative", "section_scores")}


# ---- 4. the headline case -----------------------------------------------------------------------------------------------------
def check_headline(s, data, exact=True):
    """``s``: ``episode_workers.summarise`` of a report covering all 8 ranks."""
    R, S, N = episode_workers.RANKS, episode_workers.SECTIONS, episode_workers.SAMPLES
    names = [f"section_{i:03d}" for i in range(S)]
    slow = episode_workers.EPISODE_RANK
    assert s["median_flagged"] == [], s["median_flagged"]  # identify_stragglers() names nobody
    assert s["onset_flagged"] == [] and s["period_flagged"] == []  # ... and neither do onsets and periods, where they are on
    for n in names:
        assert min(s["section_relative"][n].values()) >= 0.99, (n, s["section_relative"][n])  # medians: nobody is slow
    t = s["episodes"]
    assert s["episode_gpus"] == []  # (no kernels: the GPU episode score is NaN)
    assert all(math.isnan(v) for v in t["gpu_relative"].values()) and t["kernel_episodes"] == {}
    assert sorted(s["episode_sections"]) == names and all(v == [slow] for v in s["episode_sections"].values())
    for i, n in enumerate(names):
        for r in range(R):
            rec = t["section_episodes"][n][r]
            score = t["section_relative"][n][r]
            assert rec["window"] == N
            if r == slow:
                assert (rec["length"], rec["samples_ago"], rec["began_ago"]) == (60, N - episode_workers.END, N - episode_workers.BEGIN)
                assert abs(rec["excess"] - 1.5) <= 0.02 and abs(score - 1.0 / 1.5) <= 0.02, (n, rec, score)
                assert rec["strength"] > 0.95 and not rec["open_ended"]
            else:
                assert score >= 0.98 and rec["excess"] == 1.0, (n, r, score, rec)
                assert rec["strength"] <= 0.05, (n, r, rec)
            if exact:
                assert rec == _record(data[r, i]), (n, r)


def _report_of(cpu_backend, data, **options):
    from nvrx_straggler.reporting import ReportGenerator

    R, S, N = data.shape
    gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=True, node_name="n", episode_detection=True, **options)
    rings = cpu_backend.make_rings(R, S, N)
    names = [f"section_{s:03d}" for s in range(S)]
    rows = {n: rings.row_for(0, n) for n in names}
    for lr in range(R):
        for s, n in enumerate(names):
            rings.samples[lr * S + rows[n]] = data[lr, s]
    rings.total[:] = N
    return gen.generate_report_from_rings(rings, rows, {}, local_ranks=R)


def test_rank_slow_for_one_stretch_is_invisible_to_the_other_families_and_flagged_by_episodes(cpu_backend):
    data = episode_workers.headline_data()
    rep = _report_of(cpu_backend, data, onset_detection=True, period_detection=True, tail_quantile=0.95)
    s = episode_workers.summarise(rep)
    assert s["onsets"] and s["periods"] and s["tails"]  # (the other families were there to name somebody)
    for n, per in s["tails"]["section_relative"].items():
        assert per[episode_workers.EPISODE_RANK] >= 0.99, (n, per)  # 3 % is below the 5 % a 0.95-quantile looks at
    check_headline(s, data)


def test_a_stretch_the_whole_job_shares_flags_nobody(cpu_backend):
    data = episode_workers.jobwide_data()
    s = episode_workers.summarise(_report_of(cpu_backend, data))
    assert s["episode_sections"] == {} and s["episode_gpus"] == [] and s["median_flagged"] == []
    t = s["episodes"]
    for n, per in t["section_episodes"].items():
        for r, rec in per.items():
            assert (rec["length"], rec["samples_ago"]) == (80, episode_workers.SAMPLES - episode_workers.JOB_END), (n, r, rec)
            assert abs(rec["excess"] - 1.5) <= 0.02 and t["section_relative"][n][r] >= 0.98, (n, r, rec)


# ---- 5. lifetime and pickling -------------------------------------------------------------------------------------------------
def test_a_held_report_keeps_its_episodes_and_reports_travel(cpu_backend):
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=True, node_name="n",
                          episode_detection=True, period_detection=True, onset_detection=True, tail_quantile=0.9)
    rings = cpu_backend.make_rings(1, 8, 32)
    kernel_rows = {n: rings.row_for(1, n) for n in ("gemm", "ncclDevKernel_y")}
    section_rows = {"sec": rings.row_for(0, "sec")}
    held = []
    for w in range(4):
        v = np.full(30, 2.0 + w, dtype=np.float32)
        v[8 + w : 16 + w] *= np.float32(2.0)  # 8 slow samples from 8 + w on
        rings.push_many(kernel_rows["gemm"], v)
        rings.push_many(kernel_rows["ncclDevKernel_y"], v * 100)
        rings.push_many(section_rows["sec"], v + 0.5)
        held.append(gen.generate_report_from_rings(rings, section_rows, kernel_rows))
        rings.reset()
    assert gen._ring_plan is not None and cpu_backend.episode_score_calls == 4 and cpu_backend.onset_enable_calls == 1
    assert all(h.reads == 0 for h in cpu_backend.episode_handles)  # generate_report reads nothing
    for w in (3, 2, 1, 0):
        t = held[w].episode_scores()
        assert cpu_backend.episode_handles[w].reads == 1
        assert t["kernel_episodes"] == {"gemm": {0: {"length": 8, "samples_ago": 14 - w, "began_ago": 22 - w, "window": 30,
                                                     "inside": 2.0 * (2.0 + w), "outside": 2.0 + w, "excess": 2.0, "strength": 1.0,
                                                     "open_ended": False}}}
        assert t["section_episodes"]["sec"][0]["length"] == 8 and t["section_episodes"]["sec"][0]["strength"] == 1.0
        assert t["gpu_relative"] == {0: 1.0} and t["section_relative"] == {"sec": {0: 1.0}}  # one rank is its own reference
        assert t["gpu_scores"] == t["gpu_relative"] and t["section_scores"] == t["section_relative"]
        assert held[w].episode_scores() == t and cpu_backend.episode_handles[w].reads == 1
        assert held[w].onset_scores() and held[w].tail_scores() and held[w].period_scores()
        for clone in (pickle.loads(pickle.dumps(held[w])), copy.deepcopy(held[w])):
            assert json.dumps(clone.episode_scores()) == json.dumps(t)
            assert clone.identify_episode_stragglers() == held[w].identify_episode_stragglers()
    t = held[0].episode_scores()
    t["kernel_episodes"]["gemm"][0].clear()
    t["section_relative"]["sec"].clear()
    assert held[0].episode_scores()["kernel_episodes"]["gemm"][0] and held[0].episode_scores()["section_relative"]["sec"]
    # the dict-input path has no samples: no episodes
    from nvrx_straggler import Statistic as S

    summ = {S.MIN: 1.0, S.MAX: 2.0, S.MED: 1.5, S.AVG: 1.5, S.STD: 0.1, S.NUM: 4}
    assert gen.generate_report({"sec": summ}, {"gemm": summ}).episode_scores() == {}


def test_a_wrapped_ring_is_walked_in_time_order(cpu_backend):
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=True, node_name="n", episode_detection=True)
    rings = cpu_backend.make_rings(1, 4, 64)
    rows = {"sec": rings.row_for(0, "sec")}
    v = np.full(96, 3.0, dtype=np.float32)
    v[70:80] = 6.0  # the surviving window is v[32:]: its slow samples sit at 38 .. 47 of the window
    rings.push_many(rows["sec"], v)
    rec = gen.generate_report_from_rings(rings, rows, {}).episode_scores()["section_episodes"]["sec"][0]
    assert rec == {"length": 10, "samples_ago": 16, "began_ago": 26, "window": 64, "inside": 6.0, "outside": 3.0, "excess": 2.0,
                   "strength": 1.0, "open_ended": False}


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

    def det(episode_len_ppm):
        reporter = SimpleNamespace(_ring_plan=SimpleNamespace(fused=True, ws=None), world_size=1, _exchanged=lambda: True,
                                   _direct=None, asynchronous=False, kernel_attribution=0, tail_q_ppm=0, onset_seg_ppm=0,
                                   period_max=0, episode_len_ppm=episode_len_ppm)
        rings = SimpleNamespace(lib=SimpleNamespace(nvrx_window_report=object()))
        return SimpleNamespace(_rings=rings, reporter=reporter, _cupti_manager=Manager(), _pending_region_switch=None)

    with pytest.raises(Reached):
        straggler._Lane.build(det(0))
    assert straggler._Lane.build(det(5000)) is None


# ---- 7. the C entry points check their arguments before any device is touched ------------------------------------------------
def test_entry_points_check_their_arguments_without_a_device():
    import ctypes

    from nvrx_straggler import _native

    lib = _native.load()
    assert {"nvrx_row_episode", "nvrx_episode_score", "nvrx_episode_local"} <= {name for name, _, _ in _native.SYMBOLS}
    assert lib.nvrx_abi_version() == 2
    fake = ctypes.c_void_p(4096)

    def episode(samples=fake, counts=fake, starts=None, rows=4, stride=1024, ppm=5000, out=fake):
        return lib.nvrx_row_episode(samples, counts, starts, rows, stride, ppm, out, None)

    for ppm in (0, 333334, 500000, 1 << 30):
        assert episode(ppm=ppm) == _native.ERR_RANGE and b"min_len_ppm" in lib.nvrx_last_error()
    assert episode(rows=-1) == _native.ERR_INVALID and b"rows" in lib.nvrx_last_error()
    assert episode(stride=0) == _native.ERR_INVALID and episode(stride=1022) == _native.ERR_INVALID
    assert b"row_stride" in lib.nvrx_last_error()
    assert episode(stride=65540) == _native.ERR_RANGE
    assert episode(samples=None) == _native.ERR_INVALID and episode(counts=None) == _native.ERR_INVALID
    assert episode(out=None) == _native.ERR_INVALID and b"null" in lib.nvrx_last_error()
    assert episode(samples=ctypes.c_void_p(4100)) == _native.ERR_INVALID and b"aligned" in lib.nvrx_last_error()
    assert episode(out=ctypes.c_void_p(4104)) == _native.ERR_INVALID and b"aligned" in lib.nvrx_last_error()
    assert episode(rows=0) == 0  # nothing to do, nothing touched

    def score(episodes=fake, table=fake, R=4, K=8, S=2, first=0, n=4, scratch=fake, out=fake):
        return lib.nvrx_episode_score(episodes, table, R, K, S, first, n, scratch, out, None)

    assert score(R=0) == _native.ERR_INVALID and b"shape" in lib.nvrx_last_error()
    assert score(R=-1) == _native.ERR_INVALID and score(K=-1) == _native.ERR_INVALID and score(S=-1) == _native.ERR_INVALID
    assert score(K=70000) == _native.ERR_RANGE
    assert score(first=3, n=2) == _native.ERR_RANGE and b"outside the table" in lib.nvrx_last_error()
    assert score(first=-1) == _native.ERR_RANGE and score(n=0) == _native.ERR_RANGE and score(n=5) == _native.ERR_RANGE
    assert score(episodes=None) == _native.ERR_INVALID and score(table=None) == _native.ERR_INVALID
    assert score(out=None) == _native.ERR_INVALID
    assert score(scratch=None) == _native.ERR_INVALID and b"scratch" in lib.nvrx_last_error()

    desc = _native.ReportDesc()

    def local(ctx=fake, d=None, ppm=5000, strength=0.5, send=fake, K=8, S=2, rows_active=0):
        return lib.nvrx_episode_local(ctx, d, ppm, strength, send, K, S, rows_active, None)

    assert local(ctx=None) == _native.ERR_INVALID and local(send=None) == _native.ERR_INVALID
    assert b"null" in lib.nvrx_last_error()
    assert local(K=-1) == _native.ERR_INVALID and local(S=-1) == _native.ERR_INVALID
    assert local(K=70000) == _native.ERR_RANGE
    for ppm in (0, 333334):
        assert local(ppm=ppm) == _native.ERR_RANGE and b"min_len_ppm" in lib.nvrx_last_error()
        assert local(ppm=ppm, d=ctypes.byref(desc)) == _native.ERR_RANGE
    for strength in (-0.5, 1.5, float("nan")):
        assert local(strength=strength) == _native.ERR_RANGE and b"min_strength" in lib.nvrx_last_error()


# ---- 8. the inputs of the GPU tests: the bounds pin down the interval of (nearly) every row -----------------------------------
def _cap_check(eps, kinds, counts, len_ppm, tag):
    band = episode_workers.band_rows(eps, kinds)
    assert len(band) <= 0.02 * len(eps), (tag, band)
    for r, kind in enumerate(kinds):  # the oracle itself decides the planted tie as the definition says
        n = int(counts[r])
        if kind == "two_equal" and n:
            first = episode_workers.two_equal_first(n, min_len(len_ppm, n))
            if first:
                assert (eps[r].a, eps[r].b) == first, (tag, r, first, eps[r].a, eps[r].b)


@pytest.mark.parametrize("len_ppm", episode_workers.PPMS)
@pytest.mark.parametrize("stride", episode_workers.STRIDES)
def test_gpu_inputs_stay_within_the_cap_on_undecided_rows(stride, len_ppm):
    """No more than 2 % of a case's rows may have a second interval within 1e-10 * A of the best (or a best within that of 0):
    there the GPU tests do not compare the interval.  The oracle alone says which rows those are."""
    samples, counts, kinds = episode_workers.kernel_case(stride, len_ppm)
    _, eps = row_episode(samples, counts, len_ppm)
    _cap_check(eps, kinds, counts, len_ppm, ("stride", stride, len_ppm))
    if stride in episode_workers.ROTATION_STRIDES and len_ppm == episode_workers.LEN_PPM:
        samples, counts, starts, kinds = episode_workers.rotation_case(stride)
        _, eps = row_episode(samples, counts, len_ppm, starts)
        _cap_check(eps, kinds, counts, len_ppm, ("starts", stride))


@pytest.mark.parametrize("rows,stride", episode_workers.LAUNCHES)
def test_gpu_launch_inputs_stay_within_the_cap_on_undecided_rows(rows, stride):
    samples, counts, kinds = episode_workers.launch_case(rows, stride)
    _, eps = row_episode(samples, counts, episode_workers.LEN_PPM)
    _cap_check(eps, kinds, counts, episode_workers.LEN_PPM, ("launch", rows, stride))
