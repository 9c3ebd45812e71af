"""Tail scores, host side, on the CPU checker backend (tests/tail_oracle_backend.py): the nearest-rank index, the option's
plumbing through ReportGenerator / Detector / Report, the collectives of the tail step on gloo ranks, the headline case of
an intermittently slow rank, lifetime and pickling, and the argument checks of the three C entry points (callable without
a device).

Bounds: tails and section tail scores are compared exactly (an actual sample; one f64 quotient rounded to f32); GPU tail
scores within 2e-6 absolute, the project's tolerance for GPU scores (f64 sums in another order, values O(1))."""
import copy
import json
import math
import pickle

import numpy as np
import pytest

import tail_workers
from mp_util import run_ranks
from tail_oracle_backend import CountingTailBackend, TailOracleBackend, row_quantile, tail_rank

Q_PPMS = (500000, 900000, 950000, 990000, 999999, 623457)


@pytest.fixture
def cpu_backend():
    from nvrx_straggler import backend

    be = TailOracleBackend()
    backend.set_backend(be)
    try:
        yield be
    finally:
        backend.set_backend(None)


# ---- 1. the index, the option's values ------------------------------------------------------------------------------------
def test_nearest_rank_index_is_the_exact_rational():
    from nvrx_straggler import _native

    n = np.arange(1, 65537, dtype=np.int64)
    for q_ppm in Q_PPMS:
        got = (q_ppm * n + 999999) // 1000000 - 1
        assert [_native.tail_rank(q_ppm, int(m)) for m in (1, 2, 3, 7, 20, 8192, 10000, 65536)] == \
            [int(got[m - 1]) for m in (1, 2, 3, 7, 20, 8192, 10000, 65536)]
        exact = np.array([-(-q_ppm * int(m) // 10**6) - 1 for m in n.tolist()], dtype=np.int64)
        assert np.array_equal(got, exact), q_ppm
        assert all(_native.tail_rank(q_ppm, int(m)) == int(e) for m, e in zip(n[::97].tolist(), exact[::97].tolist()))
        assert (exact >= 0).all() and (exact < n).all()
        if q_ppm != 623457:
            q = q_ppm / 1e6
            assert exact.tolist() == [math.ceil(q * m) - 1 for m in n.tolist()], q_ppm
        assert all(tail_rank(q_ppm, int(m)) == int(e) for m, e in zip(n[::101].tolist(), exact[::101].tolist()))
    assert np.array_equal((500000 * n + 999999) // 1000000 - 1, (n - 1) // 2)  # the lower median
    # every n, through the package's own function
    for q_ppm in Q_PPMS:
        assert [_native.tail_rank(q_ppm, m) for m in range(1, 65537)] == [-(-q_ppm * m // 10**6) - 1 for m in range(1, 65537)]


def test_option_values(cpu_backend, monkeypatch):
    from nvrx_straggler import Detector, _native
    from nvrx_straggler.reporting import ReportGenerator

    assert _native.tail_q_ppm(0.95) == 950000 and _native.tail_q_ppm(0) == 0 and _native.tail_q_ppm(None) == 0
    assert _native.tail_q_ppm(0.5) == 500000 and _native.tail_q_ppm(0.999999) == 999999 and _native.tail_q_ppm("0.9") == 900000
    for bad in (0.3, 1.0, "x", -0.9, 0.4999):
        with pytest.raises(ValueError, match="tail_quantile"):
            ReportGenerator(["relative_perf_scores"], tail_quantile=bad)
    with pytest.raises(ValueError, match="tail_quantile.*relative_perf_scores"):
        ReportGenerator(["individual_perf_scores"], tail_quantile=0.9)
    with pytest.raises(ValueError, match="tail_quantile.*relative_perf_scores"):
        Detector.initialize(scores_to_compute=["individual_perf_scores"], tail_quantile=0.9)
    assert not Detector.initialized
    assert ReportGenerator(["relative_perf_scores"], tail_quantile=0.95).tail_q_ppm == 950000
    assert ReportGenerator(["individual_perf_scores"]).tail_q_ppm == 0
    # the environment variable is the Detector's default, read only when the argument is None
    monkeypatch.setenv("NVRX_TAIL_QUANTILE", "0.9")
    Detector.initialize(node_name="n0")
    try:
        assert Detector.reporter.tail_q_ppm == 900000
    finally:
        Detector.shutdown()
    Detector.initialize(node_name="n0", tail_quantile=0)
    try:
        assert Detector.reporter.tail_q_ppm == 0
    finally:
        Detector.shutdown()
    Detector.initialize(node_name="n0", tail_quantile=0.99)
    try:
        assert Detector.reporter.tail_q_ppm == 990000
    finally:
        Detector.shutdown()
    monkeypatch.setenv("NVRX_TAIL_QUANTILE", "most")
    with pytest.raises(ValueError, match="tail_quantile"):
        Detector.initialize(node_name="n0")
    assert not Detector.initialized
    monkeypatch.setenv("NVRX_TAIL_QUANTILE", "0.3")
    with pytest.raises(ValueError, match="tail_quantile"):
        Detector.initialize(node_name="n0")
    assert not Detector.initialized
    monkeypatch.delenv("NVRX_TAIL_QUANTILE")
    Detector.initialize(node_name="n0")
    try:
        assert Detector.reporter.tail_q_ppm == 0
    finally:
        Detector.shutdown()


def test_option_needs_a_backend_with_tail_score():
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator
    from oracle_backend import OracleBackend

    backend.set_backend(OracleBackend())
    try:
        with pytest.raises(RuntimeError, match="no tail scores"):
            ReportGenerator(["relative_perf_scores"], tail_quantile=0.9)
        ReportGenerator(["relative_perf_scores"], tail_quantile=0.0)
    finally:
        backend.set_backend(None)


# ---- 2. off by default: nothing is called -----------------------------------------------------------------------------------
@pytest.mark.parametrize("emulate_fused,asynchronous", [(False, False), (True, False), (True, True)])
def test_default_is_off_and_calls_nothing(emulate_fused, asynchronous):
    from nvrx_straggler import Detector
    from nvrx_straggler import Statistic as S
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator

    be = CountingTailBackend(emulate_fused=emulate_fused)
    backend.set_backend(be)
    try:
        gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=True, node_name="n",
                              asynchronous=asynchronous)
        assert gen.tail_q_ppm == 0
        summ = {S.MIN: 1.0, S.MAX: 2.0, S.MED: 1.5, S.AVG: 1.5, S.STD: 0.1, S.NUM: 4}
        rep = gen.generate_report({"sec": summ}, {"k": summ})
        assert rep.tail_scores() == {} and pickle.loads(pickle.dumps(rep)).tail_scores() == {}
        assert rep.identify_tail_stragglers() == {"straggler_gpus_relative": set(), "straggler_sections_relative": {}}
        rings = be.make_rings(1, 8, 16)
        krow, srow = rings.row_for(1, "kern"), rings.row_for(0, "sec")
        kernel_rows, section_rows = {"kern": krow}, {"sec": srow}
        for i in range(3):
            rings.push_many(krow, [1.0 + i, 2.0, 3.0])
            rings.push_many(srow, [5.0, 6.0])
            rep = gen.generate_report_from_rings(rings, section_rows, kernel_rows)
            rings.reset()
            assert rep.tail_scores() == {}
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
                    sec.cpu_elapsed_times.extend(np.full(5, value, dtype=np.float32))
                rep = Detector.generate_report()
                assert rep.tail_scores() == {}
                assert set(rep.section_relative_perf_scores) == {"a", "b"}
        finally:
            Detector.shutdown()
        assert be.tail_calls == 0
    finally:
        backend.set_backend(None)


# ---- 3. the tail step's collectives on gloo ranks -----------------------------------------------------------------------------
def _expected_tails(res, world, i, q_ppm):
    """name -> {rank: tail} of report i from what every rank pushed (collective kernels are not exchanged)."""
    exp = {}
    for r in range(world):
        for key, vals in res[r]["reports"][i]["pushed"].items():
            if "ncclDev" in key:
                continue
            v = np.array(vals, dtype=np.float32)[None, :]
            exp.setdefault(key, {})[r] = float(row_quantile(v, [v.shape[1]], q_ppm)[0])
    return exp


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("gather_on_rank0", [True, False])
def test_every_rank_issues_the_same_collectives_and_tails_are_right(world, gather_on_rank0):
    q_ppm = 900000
    res = run_ranks(tail_workers.ring_reports_recorded, world, timeout=300, gather_on_rank0=gather_on_rank0, q=q_ppm / 1e6)
    for i in range(6):
        seqs = [res[r]["calls"][i] for r in range(world)]
        assert all(s == seqs[0] for s in seqs), (i, seqs)
        rows = [c for c in seqs[0] if c[0] == "rows"]
        assert len(rows) >= 2 and rows[-1][1] < rows[-2][1], (i, seqs[0])  # the tail rows travel last: [K+S] against [L]
    assert all(res[r]["tail_local_calls"] == 6 for r in range(world))
    for r in range(world):
        assert res[r]["tail_score_calls"] == (6 if (r == 0 or not gather_on_rank0) else 0)
    for i in range(6):
        exp = _expected_tails(res, world, i, q_ppm)
        for r in range(world):
            entry = res[r]["reports"][i]
            if gather_on_rank0 and r != 0:
                assert entry["tails"] is None
                continue
            t = entry["tails"]
            assert entry["pickled_same"] and t["quantile"] == 0.9
            covered = list(range(world)) if gather_on_rank0 else [r]
            assert sorted(t["gpu_relative"]) == covered
            for kind, got in (("section", t["section_tails"]), ("kernel", t["kernel_tails"])):
                want = {k.split(":", 1)[1]: {rr: v for rr, v in per.items() if rr in covered}
                        for k, per in exp.items() if k.startswith(kind)}
                want = {k: v for k, v in want.items() if v}
                # (the report that meets a new name syncs names and runs its score round again: the name has an id by then)
                assert got == want, (i, r, kind, got, want)
            # section tail scores: the fastest rank's tail over this rank's, NaN where some rank lacks the section
            for name, per in t["section_relative"].items():
                tails = exp.get(f"section:{name}", {})
                for rr, score in per.items():
                    if len(tails) < world or rr not in tails:
                        assert math.isnan(score), (i, r, name, rr, score)
                    else:
                        ref = np.float32(min(tails.values()))
                        assert score == float(np.float32(np.float64(ref) / np.float64(np.float32(tails[rr])))), (i, name, rr)
            # GPU tail score: kernels every rank has (k0; k_new is rank 0's alone and has no reference)
            k0 = exp["kernel:k0"]
            for rr in covered:
                want = float(np.float32(min(k0.values()))) / k0[rr]
                assert abs(t["gpu_relative"][rr] - want) <= 2e-6, (i, rr, t["gpu_relative"][rr], want)


# ---- 4. the headline case -----------------------------------------------------------------------------------------------------
def test_intermittently_slow_rank_is_invisible_to_medians_and_flagged_by_tails(cpu_backend):
    from nvrx_straggler.reporting import ReportGenerator

    data = tail_workers.headline_data()
    gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=True, node_name="n", tail_quantile=0.95)
    rings = cpu_backend.make_rings(8, 64, 10000)
    names = [f"section_{s:03d}" for s in range(64)]
    rows = {n: rings.row_for(0, n) for n in names}
    for lr in range(8):
        for s, n in enumerate(names):
            rings.samples[lr * 64 + rows[n]] = data[lr, s]
    rings.total[:] = 10000
    rep = gen.generate_report_from_rings(rings, rows, {}, local_ranks=8)
    found = rep.identify_stragglers()
    assert found["straggler_gpus_relative"] == set() and found["straggler_sections_relative"] == {}
    assert min(min(v.values()) for v in rep.section_relative_perf_scores.values()) > 0.99  # medians: nobody is slow
    tails = rep.tail_scores()
    flagged = rep.identify_tail_stragglers()
    assert flagged["straggler_gpus_relative"] == set()  # (no kernels: the GPU tail score is NaN)
    assert sorted(flagged["straggler_sections_relative"]) == names
    assert all({s.rank for s in v} == {3} for v in flagged["straggler_sections_relative"].values())
    k = tail_rank(950000, 10000)
    for s, n in enumerate(names):
        for r in range(8):
            assert tails["section_tails"][n][r] == float(np.sort(data[r, s])[k]), (n, r)
            score = tails["section_relative"][n][r]
            if r == 3:
                assert 0.68 <= score <= 0.70, (n, score)
            else:
                assert score >= 0.99, (n, r, score)
    assert all(math.isnan(v) for v in tails["gpu_relative"].values()) and tails["kernel_tails"] == {}


# ---- 5. lifetime and pickling -------------------------------------------------------------------------------------------------
def test_a_held_report_keeps_its_tails_and_reports_travel(cpu_backend):
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=True, node_name="n",
                          tail_quantile=0.9)
    rings = cpu_backend.make_rings(1, 8, 16)
    kernel_rows = {n: rings.row_for(1, n) for n in ("gemm", "ncclDevKernel_y")}
    section_rows = {"sec": rings.row_for(0, "sec")}
    held = []
    windows = [np.arange(1, 11, dtype=np.float32) * (w + 1) for w in range(4)]
    for v in windows:
        rings.push_many(kernel_rows["gemm"], v)
        rings.push_many(kernel_rows["ncclDevKernel_y"], v * 100)
        rings.push_many(section_rows["sec"], v[::-1] + 0.5)
        held.append(gen.generate_report_from_rings(rings, section_rows, kernel_rows))
        rings.reset()
    assert gen._ring_plan is not None and cpu_backend.tail_score_calls == 4
    assert all(h.reads == 0 for h in cpu_backend.handles)  # generate_report reads nothing
    for w in (3, 2, 1, 0):
        t = held[w].tail_scores()
        assert cpu_backend.handles[w].reads == 1
        assert t["quantile"] == 0.9
        assert t["kernel_tails"] == {"gemm": {0: 9.0 * (w + 1)}}  # rank k = ceil(0.9 * 10) - 1 = 8 of 1..10, scaled
        assert t["section_tails"] == {"sec": {0: 9.0 * (w + 1) + 0.5}}
        assert t["gpu_relative"] == {0: 1.0} and t["section_relative"] == {"sec": {0: 1.0}}
        assert held[w].tail_scores() == t and cpu_backend.handles[w].reads == 1
        for clone in (pickle.loads(pickle.dumps(held[w])), copy.deepcopy(held[w])):
            assert json.dumps(clone.tail_scores()) == json.dumps(t)
            assert clone.identify_tail_stragglers() == held[w].identify_tail_stragglers()
    t = held[0].tail_scores()
    t["kernel_tails"].clear()
    t["section_relative"]["sec"].clear()
    assert held[0].tail_scores()["kernel_tails"] and held[0].tail_scores()["section_relative"]["sec"]
    # the dict-input path has no samples: no tails
    from nvrx_straggler import Statistic as S

    summ = {S.MIN: 1.0, S.MAX: 2.0, S.MED: 1.5, S.AVG: 1.5, S.STD: 0.1, S.NUM: 4}
    assert gen.generate_report({"sec": summ}, {"gemm": summ}).tail_scores() == {}


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

    def det(q_ppm):
        reporter = SimpleNamespace(_ring_plan=SimpleNamespace(fused=True, ws=None), world_size=1, _exchanged=lambda: True,
                                   _direct=None, asynchronous=False, kernel_attribution=0, tail_q_ppm=q_ppm)
        rings = SimpleNamespace(lib=SimpleNamespace(nvrx_window_report=object()))
        return SimpleNamespace(_rings=rings, reporter=reporter, _cupti_manager=Manager(), _pending_region_switch=None)

    with pytest.raises(Reached):
        straggler._Lane.build(det(0))
    assert straggler._Lane.build(det(900000)) is None


# ---- 7. the C entry points check their arguments before any device is touched ------------------------------------------------
def test_entry_points_check_their_arguments_without_a_device():
    import ctypes

    from nvrx_straggler import _native

    lib = _native.load()
    assert {"nvrx_row_quantile", "nvrx_tail_score", "nvrx_tail_local"} <= {name for name, _, _ in _native.SYMBOLS}
    assert lib.nvrx_abi_version() == 2
    fake = ctypes.c_void_p(4096)

    def quant(samples=fake, counts=fake, rows=4, stride=1024, q=950000, out=fake):
        return lib.nvrx_row_quantile(samples, counts, rows, stride, q, out, None)

    for q in (0, 499999, 1000000, 4000000000):
        assert quant(q=q) == _native.ERR_RANGE and b"q_ppm" in lib.nvrx_last_error()
    assert quant(rows=-1) == _native.ERR_INVALID and b"rows" in lib.nvrx_last_error()
    assert quant(stride=0) == _native.ERR_INVALID and quant(stride=1022) == _native.ERR_INVALID
    assert b"row_stride" in lib.nvrx_last_error()
    assert quant(stride=65540) == _native.ERR_RANGE
    assert quant(samples=None) == _native.ERR_INVALID and quant(counts=None) == _native.ERR_INVALID
    assert quant(out=None) == _native.ERR_INVALID and b"null" in lib.nvrx_last_error()
    assert quant(samples=ctypes.c_void_p(4100)) == _native.ERR_INVALID and b"aligned" in lib.nvrx_last_error()
    assert quant(rows=0) == 0  # nothing to do, nothing touched

    def score(tails=fake, table=fake, R=4, K=8, S=2, first=0, n=4, scratch=fake, out=fake):
        return lib.nvrx_tail_score(tails, table, R, K, S, first, n, scratch, out, None)

    assert score(R=0) == _native.ERR_INVALID and b"shape" in lib.nvrx_last_error()
    assert score(R=-1) == _native.ERR_INVALID and score(K=-1) == _native.ERR_INVALID and score(S=-1) == _native.ERR_INVALID
    assert score(K=70000) == _native.ERR_RANGE
    assert score(first=3, n=2) == _native.ERR_RANGE and b"outside the table" in lib.nvrx_last_error()
    assert score(first=-1) == _native.ERR_RANGE and score(n=0) == _native.ERR_RANGE and score(n=5) == _native.ERR_RANGE
    assert score(tails=None) == _native.ERR_INVALID and score(table=None) == _native.ERR_INVALID
    assert score(out=None) == _native.ERR_INVALID
    assert score(scratch=None) == _native.ERR_INVALID and b"scratch" in lib.nvrx_last_error()

    desc = _native.ReportDesc()

    def local(ctx=fake, d=None, q=950000, send=fake, K=8, S=2, rows_active=0):
        return lib.nvrx_tail_local(ctx, d, q, send, K, S, rows_active, None)

    assert local(ctx=None) == _native.ERR_INVALID and local(send=None) == _native.ERR_INVALID
    assert b"null" in lib.nvrx_last_error()
    assert local(K=-1) == _native.ERR_INVALID and local(S=-1) == _native.ERR_INVALID
    assert local(K=70000) == _native.ERR_RANGE
    for q in (0, 499999, 1000000):
        assert local(q=q) == _native.ERR_RANGE and b"q_ppm" in lib.nvrx_last_error()
        assert local(q=q, d=ctypes.byref(desc)) == _native.ERR_RANGE
