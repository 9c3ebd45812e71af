"""Kernel attribution, host side, on the CPU checker backend (tests/attribution_oracle_backend.py): the option's plumbing
through ReportGenerator / Report, coverage and names in both gather modes against the golden scenarios of scoring.json,
lifetime, pickling, and the argument checks of the two C entry points (callable without a device).

Tolerances: shares / deficit / explained absolute 2e-6 (the bound tests/test_gpu_score.py uses for GPU scores: f64 sums in
another order, values O(1)); against the reference's golden scores 1e-4, the project's score tolerance.  Kernel names and
their order are compared exactly everywhere."""
import json
import math
import pickle

import numpy as np
import pytest

import attribution_workers
from attribution_oracle_backend import (AttributionOracleBackend, CountingOracleBackend, attribute_table,
                                        expected_from_summaries)
from mp_util import run_ranks
from util import load_golden
from workers import _summ

_SCENARIOS = load_golden("scoring.json")["scenarios"]
_TOL, _GOLDEN_TOL = 2e-6, 1e-4


@pytest.fixture
def cpu_backend():
    from nvrx_straggler import backend

    be = AttributionOracleBackend()
    backend.set_backend(be)
    try:
        yield be
    finally:
        backend.set_backend(None)


def _check_scenario(g, res):
    """``res[rank][step]`` = attribution_workers.scoring_scenario_attributed's output; every report, rank and family."""
    sc = g["scenario"]
    world, steps = sc["world_size"], sc["steps"]
    families = [f for f, key in (("relative", "relative_perf_scores"), ("individual", "individual_perf_scores"))
                if key in sc["scores_to_compute"]]
    checked = nan_headers = 0
    for r in range(world):
        for t in range(len(steps)):
            got = res[r][t]
            golden = g["per_rank"][r]["reports"][t]
            assert (got is None) == (golden is None), (sc["name"], r, t)
            if got is None:
                continue
            ex = got["explain"]
            assert got["pickled_same"]
            json.dumps(ex)  # plain dicts / lists / floats / str
            assert sorted(ex) == sorted(families), (sc["name"], ex.keys())
            covered = list(range(world)) if sc["gather_on_rank0"] else [r]
            for fam in families:
                assert sorted(ex[fam]) == covered, (sc["name"], fam, r, t)
                for rr in covered:
                    e = ex[fam][rr]
                    tag = (sc["name"], fam, r, t, rr)
                    gscore = golden[f"gpu_{fam}_perf_scores"][str(rr)]
                    exp = expected_from_summaries(steps, t, rr, world, got["kernel_ids"], fam)
                    assert all("ncclDev" not in k["kernel"] for k in e["kernels"]), tag
                    if exp is None:
                        assert math.isnan(gscore), tag  # the reference reports NaN exactly where nothing is eligible
                        assert math.isnan(e["deficit"]) and e["kernels"] == [] and e["num_kernels"] == 0, tag
                        nan_headers += 1
                        continue
                    deficit, ranked = exp
                    assert not math.isnan(gscore), tag
                    assert abs(e["deficit"] - (1.0 - gscore)) <= _GOLDEN_TOL, (tag, e["deficit"], gscore)
                    assert abs(e["deficit"] - deficit) <= _TOL, tag
                    assert e["num_kernels"] == len(ranked) <= 16, tag
                    assert [k["kernel"] for k in e["kernels"]] == [name for name, *_ in ranked], (tag, e["kernels"], ranked)
                    for k, (_, share, score, lost) in zip(e["kernels"], ranked):
                        assert abs(k["share"] - share) <= _TOL, tag
                        assert k["score"] == float(np.float32(score)) and k["lost_us"] == float(np.float32(lost)), tag
                    # all eligible kernels are listed (N = 16 >= their number): the shares add up to the deficit
                    assert abs(sum(k["share"] for k in e["kernels"]) - e["deficit"]) <= _TOL, tag
                    assert abs(e["explained"] - e["deficit"]) <= _TOL, tag
                    checked += 1
    return checked, nan_headers


@pytest.mark.parametrize("world", [2, 4, 8])
def test_golden_scenarios_on_gloo_ranks(world):
    """Every multi-rank scenario of scoring.json, both gather modes, dict-input path, N = 16."""
    batch = [g for g in _SCENARIOS if g["scenario"]["world_size"] == world]
    assert batch
    res = run_ranks(attribution_workers.scoring_scenarios_attributed_batch, world, timeout=300,
                    scenarios=[g["scenario"] for g in batch])
    total = nans = 0
    for i, g in enumerate(batch):
        c, n = _check_scenario(g, [res[r][i] for r in range(world)])
        total, nans = total + c, nans + n
    assert total > 0
    if world == 4:
        assert nans > 0  # rank_without_kernels: NaN headers


def test_individual_history_in_one_process(cpu_backend):
    g = next(s for s in _SCENARIOS if s["scenario"]["name"] == "indiv_history_1rank")
    res = attribution_workers.scoring_scenario_attributed(0, 1, g["scenario"], cpu=False)
    assert len(res) == 7
    checked, _ = _check_scenario(g, [res])
    assert checked == 7
    assert cpu_backend.attribute_calls == 7


def test_common_and_unique_kernels_lists_only_the_common_ones(cpu_backend):
    """Relative family: a kernel some rank lacks has no reference and is skipped; the individual family lists it."""
    from nvrx_straggler import Statistic as S
    from nvrx_straggler.reporting import ReportGenerator

    def summ(med, n=10):
        return {S.MIN: med, S.MAX: med, S.MED: med, S.AVG: med, S.STD: 0.0, S.NUM: n}

    # one process: the table has one rank, so "common" is trivially everything; drive the operator on a 2-rank table instead
    K, S_ = 3, 0
    L = 2 * K + K + 1
    T = np.zeros((2, L), dtype=np.float32)
    T[0, :K] = [2.0, 4.0, 1.0]
    T[1, :K] = [1.0, -1.0, 1.0]          # rank 1 lacks kernel 1
    T[:, K : 2 * K] = [[1.0, 2.0, 1.0], [1.0, np.nan, 1.0]]
    T[:, 2 * K : 3 * K] = [[20.0, 40.0, 10.0], [10.0, 0.0, 10.0]]
    rec = attribute_table(T, K, S_, 2, True, True)
    ids = rec.view(np.int32)[:, :, 1:, 0]
    assert ids[0, 1].tolist() == [0, 2]      # relative: kernel 1 is not common; kernel 2 has lost 0 and is listed second
    assert ids[0, 0].tolist() == [1, 0]      # individual: kernel 1 lost 20 us, kernel 0 lost 10 us
    assert ids[1, 1].tolist() == [0, 2]      # the fastest rank: both lost exactly 0.0 -> the lower id first
    assert rec[0, 1, 0, 2] == 2 and rec[0, 0, 0, 2] == 3
    gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=False, node_name="n", kernel_attribution=2)
    rep = gen.generate_report({}, {"a": summ(2.0), "ncclDevKernel_x": summ(50.0), "b": summ(3.0)})
    ex = rep.explain_gpu_scores()
    assert list(ex) == ["relative"] and list(ex["relative"]) == [0]
    assert [k["kernel"] for k in ex["relative"][0]["kernels"]] == ["a", "b"]  # both lost 0.0: id order; no collective kernel
    assert ex["relative"][0]["deficit"] == 0.0 and ex["relative"][0]["num_kernels"] == 2


def test_default_is_off_and_calls_nothing():
    from nvrx_straggler import Statistic as S
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator

    be = CountingOracleBackend()
    backend.set_backend(be)
    try:
        gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=True, node_name="n")
        assert gen.kernel_attribution == 0
        summ = {S.MIN: 1.0, S.MAX: 2.0, S.MED: 1.5, S.AVG: 1.5, S.STD: 0.1, S.NUM: 4}
        rep = gen.generate_report({"sec": summ}, {"k": summ})
        assert rep.explain_gpu_scores() == {} and pickle.loads(pickle.dumps(rep)).explain_gpu_scores() == {}
        # ring path: the general report, then two planned ones
        rings = be.make_rings(1, 8, 16)
        krow, srow = rings.row_for(1, "kern"), rings.row_for(0, "sec")
        kernel_rows, section_rows = {"kern": krow}, {"sec": srow}
        for i in range(3):
            rings.push_many(krow, [1.0 + i, 2.0, 3.0])
            rings.push_many(srow, [5.0, 6.0])
            rep = gen.generate_report_from_rings(rings, section_rows, kernel_rows)
            rings.reset()
            assert rep.explain_gpu_scores() == {}
            assert 0 in rep.gpu_individual_perf_scores
        assert gen._ring_plan is not None
        assert be.attribute_calls == 0
    finally:
        backend.set_backend(None)


def test_option_needs_a_backend_with_attribute_and_a_valid_n():
    from nvrx_straggler import Detector, backend
    from nvrx_straggler.reporting import ReportGenerator
    from oracle_backend import OracleBackend

    backend.set_backend(OracleBackend())
    try:
        with pytest.raises(RuntimeError, match="no kernel attribution"):
            ReportGenerator(["relative_perf_scores"], kernel_attribution=3)
        with pytest.raises(RuntimeError, match="no kernel attribution"):
            Detector.initialize(kernel_attribution=3)
        assert not Detector.initialized
        ReportGenerator(["relative_perf_scores"], kernel_attribution=0)
    finally:
        backend.set_backend(None)
    backend.set_backend(AttributionOracleBackend())
    try:
        for bad in (-1, 17):
            with pytest.raises(ValueError, match="kernel_attribution"):
                ReportGenerator(["relative_perf_scores"], kernel_attribution=bad)
    finally:
        backend.set_backend(None)


def test_environment_variable_is_the_detectors_default(cpu_backend, monkeypatch):
    from nvrx_straggler import Detector

    monkeypatch.setenv("NVRX_KERNEL_ATTRIBUTION", "5")
    Detector.initialize(node_name="n0")
    try:
        assert Detector.reporter.kernel_attribution == 5
    finally:
        Detector.shutdown()
    Detector.initialize(node_name="n0", kernel_attribution=0)
    try:
        assert Detector.reporter.kernel_attribution == 0
    finally:
        Detector.shutdown()
    monkeypatch.setenv("NVRX_KERNEL_ATTRIBUTION", "many")
    with pytest.raises(ValueError, match="NVRX_KERNEL_ATTRIBUTION"):
        Detector.initialize(node_name="n0")
    assert not Detector.initialized


def test_ring_path_and_a_report_held_across_the_next_one(cpu_backend):
    """Ring path in one process (general report, then planned ones): a report that is kept UNREAD while the next report runs
    still explains its own window; pickle / json carry the explanation."""
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=True, node_name="n",
                          kernel_attribution=2)
    rings = cpu_backend.make_rings(1, 8, 16)
    rows = {n: rings.row_for(1, n) for n in ("fast", "slow", "ncclDevKernel_y")}
    srow = rings.row_for(0, "sec")
    kernel_rows, section_rows = dict(rows), {"sec": srow}
    held = []
    for window, slow_us in enumerate((10.0, 10.0, 30.0, 50.0)):
        rings.push_many(rows["fast"], [5.0] * 4)
        rings.push_many(rows["slow"], [slow_us] * 4)
        rings.push_many(rows["ncclDevKernel_y"], [1000.0] * 4)
        rings.push_many(srow, [7.0, 8.0])
        held.append(gen.generate_report_from_rings(rings, section_rows, kernel_rows))
        rings.reset()
    assert gen._ring_plan is not None and cpu_backend.attribute_calls == 4
    # read in reverse order, long after their windows
    for window in (3, 2, 1, 0):
        slow_us = (10.0, 10.0, 30.0, 50.0)[window]
        ex = held[window].explain_gpu_scores()
        ind = ex["individual"][0]
        assert [k["kernel"] for k in ind["kernels"]] == (["slow", "fast"] if slow_us > 10.0 else ["fast", "slow"]), window
        lost = 4 * slow_us * (1.0 - 10.0 / slow_us)
        assert ind["kernels"][0]["lost_us"] == pytest.approx(lost if slow_us > 10.0 else 0.0)
        assert abs(ind["deficit"] - (1.0 - held[window].gpu_individual_perf_scores[0])) <= 1e-6
        assert ex["relative"][0]["deficit"] == 0.0  # one rank: it is its own reference
        assert ind["num_kernels"] == 2
        clone = pickle.loads(pickle.dumps(held[window]))
        assert json.dumps(clone.explain_gpu_scores()) == json.dumps(ex)
    # the caller may do what it likes with the result
    ex = held[3].explain_gpu_scores()
    ex["individual"][0]["kernels"].clear()
    assert len(held[3].explain_gpu_scores()["individual"][0]["kernels"]) == 2


def test_entry_points_check_their_arguments_without_a_device():
    """top_n 0 or > 16, ranks outside the table -> NVRX_ERR_RANGE; bad shapes / null pointers -> NVRX_ERR_INVALID; all
    before any device is touched."""
    import ctypes

    from nvrx_straggler import _native

    lib = _native.load()
    assert {"nvrx_attribute", "nvrx_report_attribute"} <= {name for name, _, _ in _native.SYMBOLS}
    assert _native.ATTR_MAX_TOP == 16 and _native.attr_words(3, 5) == 3 * 2 * 6 * 4
    fake = ctypes.c_void_p(4096)

    def call(R=4, K=8, S=2, first=0, n=4, top=5, table=fake, out=fake, scratch=fake, rel=1):
        return lib.nvrx_attribute(table, R, K, S, first, n, top, 1, rel, scratch, out, None)

    assert call(top=0) == _native.ERR_RANGE and b"top_n" in lib.nvrx_last_error()
    assert call(top=17) == _native.ERR_RANGE
    assert call(first=3, n=2) == _native.ERR_RANGE and b"outside the table" in lib.nvrx_last_error()
    assert call(first=-1) == _native.ERR_RANGE
    assert call(n=0) == _native.ERR_RANGE
    assert call(n=5) == _native.ERR_RANGE
    assert call(R=0) == _native.ERR_INVALID
    assert call(K=-1) == _native.ERR_INVALID
    assert call(K=70000) == _native.ERR_RANGE
    assert call(table=None) == _native.ERR_INVALID
    assert call(out=None) == _native.ERR_INVALID
    assert call(out=ctypes.c_void_p(4100)) == _native.ERR_INVALID and b"aligned" in lib.nvrx_last_error()
    assert call(scratch=None) == _native.ERR_INVALID and b"scratch" in lib.nvrx_last_error()
    desc = _native.ReportDesc()
    desc.R, desc.K, desc.S = 4, 8, 2
    assert lib.nvrx_report_attribute(None, ctypes.byref(desc), 0, 4, 5, fake) == _native.ERR_INVALID
    assert lib.nvrx_report_attribute(fake, None, 0, 4, 5, fake) == _native.ERR_INVALID
    assert lib.nvrx_report_attribute(fake, ctypes.byref(desc), 0, 4, 0, fake) == _native.ERR_RANGE
    assert lib.nvrx_report_attribute(fake, ctypes.byref(desc), 2, 3, 5, fake) == _native.ERR_RANGE
    assert lib.nvrx_report_attribute(fake, ctypes.byref(desc), 0, 4, 5, None) == _native.ERR_INVALID


def test_callback_names_the_kernels_of_a_flagged_rank(cpu_backend, caplog):
    """StragglerDetectionCallback: with attribution on, the warning about a flagged GPU is followed by a line naming that rank's
    kernels above the reference pace; with it off (explain_gpu_scores() == {}) the digest logs exactly what it logged before."""
    import logging

    from nvidia_resiliency_ext.ptl_resiliency.straggler_det_callback import StragglerDetectionCallback
    from nvrx_straggler import Statistic as S
    from nvrx_straggler.reporting import ReportGenerator

    def summ(med, n=10):
        return {S.MIN: med, S.MAX: med, S.MED: med, S.AVG: med, S.STD: 0.0, S.NUM: n}

    def transcript(kernel_attribution):
        gen = ReportGenerator(["individual_perf_scores"], gather_on_rank0=True, node_name="n0", kernel_attribution=kernel_attribution)
        gen.generate_report({}, {"gemm": summ(10.0), "copy": summ(2.0), "norm": summ(1.0)})
        rep = gen.generate_report({}, {"gemm": summ(40.0), "copy": summ(2.0), "norm": summ(1.5)})
        cb = StragglerDetectionCallback(report_time_interval=1.0, calc_relative_gpu_perf=False, calc_individual_gpu_perf=True,
                                        num_gpu_perf_scores_to_print=0, gpu_relative_perf_threshold=0.7,
                                        gpu_individual_perf_threshold=0.7, stop_if_detected=False, enable_ptl_logging=False,
                                        logger_name="test.attribution.callback")
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="test.attribution.callback"):
            assert cb._digest(None, rep) is True
        return [r.getMessage() for r in caplog.records]

    off, on = transcript(0), transcript(2)
    assert len(off) == 1 and "Some GPUs performance dropped." in off[0]
    assert on[0] == off[0] and len(on) == 2
    line = on[1]
    assert "rank 0 individual GPU score deficit" in line and "top kernels: gemm (share" in line
    assert line.index("gemm") < line.index("norm") and "copy" not in line  # two listed, largest loss first; copy lost nothing
    assert "lost 300 us" in line  # 10 x 40 us x (1 - 10 / 40)
