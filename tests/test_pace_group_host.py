"""Pace scores per peer group, host side, on the CPU checker backend (tests/pace_group_oracle_backend.py): the NumPy restatement
against the job-wide one (one group, ``min_peers = 1``: word for word), the pipeline scenario of the feature's sketch (8 ranks x
120 kernels, seeds 0, 1 and 2026, ``block:4`` and ``block:2``) through ReportGenerator, singleton groups and the threshold
rule, the option's plumbing through ReportGenerator / Detector / FoldedJob's keyword / the Lightning callback, that nothing new
is called with the option off, all attachment sites, that the option adds no collective on gloo ranks, lifetime and pickling.

Bounds: everything here runs on the restatement itself, so records are compared exactly."""
import copy
import json
import math
import pickle

import numpy as np
import pytest

import pace_group_workers as workers
from mp_util import run_ranks
from pace_group_oracle_backend import (CountingPaceGroupBackend, PaceGroupOracleBackend, pace_group_scores_table, threshold)
from pace_oracle_backend import pace_scores_table
from pace_workers import ranks_named


@pytest.fixture
def cpu_backend():
    from nvrx_straggler import backend

    be = PaceGroupOracleBackend()
    backend.set_backend(be)
    try:
        yield be
    finally:
        backend.set_backend(None)


def _groups(labels):
    from nvrx_straggler.backend import PeerGroups

    return PeerGroups(list(labels))


def _small_table(rng, R, K, S):
    KS = K + S
    T = np.zeros((R, 2 * KS + K + 1), dtype=np.float32)
    T[:, :KS] = rng.choice(np.array([0.0, 1.0, 2.0, 3.0, 4.0, 6.0, np.inf, -1.0, np.nan], dtype=np.float32), (R, KS),
                           p=[0.05, 0.2, 0.2, 0.15, 0.1, 0.1, 0.05, 0.1, 0.05])
    T[:, 2 * KS : 2 * KS + K] = rng.integers(1, 50, (R, K))
    return T


# ---- 1. the restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,K,S,min_ranks", [(1, 3, 0, 1), (2, 2, 2, 2), (5, 4, 3, 2), (6, 0, 5, 3), (7, 9, 1, 4), (9, 6, 6, 1)])
def test_one_group_of_all_ranks_is_the_job_wide_restatement_word_for_word(R, K, S, min_ranks):
    rng = np.random.default_rng(R * 100 + K * 10 + S)
    g = _groups([0] * R)
    assert (g.G, g.max_size) == (1, R)
    for _ in range(10):
        T = _small_table(rng, R, K, S)
        first = int(rng.integers(0, R))
        n = int(rng.integers(1, R - first + 1))
        cols, recs, terms = pace_group_scores_table(T, K, S, g.host, 1, R, first, n, min_ranks, 1)
        wcols, wrecs, wterms = pace_scores_table(T, K, S, first, n, min_ranks)
        assert cols.shape == (1, K + S, 4) and np.array_equal(cols[0], wcols)
        assert np.array_equal(recs, wrecs) and np.array_equal(terms, wterms)


def test_restatement_on_a_hand_worked_table_with_interleaved_groups():
    K, S = 2, 1
    T = np.zeros((6, 2 * (K + S) + K + 1), dtype=np.float32)
    # groups by rank: a b a b a c -- a = {0, 2, 4}, b = {1, 3}, c = {5}
    T[:, 0] = [10.0, 100.0, 20.0, 200.0, 40.0, 7.0]
    T[:, 1] = [8.0, -1.0, -1.0, 50.0, 4.0, 7.0]    # a: two present (below min(4, 3) = 3); b: one present (below min_peers)
    T[:, 2] = [5.0, 5.0, 5.0, 6.0, 5.0, 5.0]
    T[:, 6:8] = [[1.0, 2.0]] * 6
    g = _groups("ababac")
    assert g.labels == ("a", "b", "c") and g.max_size == 3 and g.members(0) == [0, 2, 4]
    cols, recs, _ = pace_group_scores_table(T, K, S, g.host, g.G, g.max_size, min_ranks=4, min_peers=2)
    f, cf = recs.view(np.float32), cols.view(np.float32)
    assert cols[:, :, 1:].tolist() == [[[3, 1, 1], [2, 1, 0], [3, 0, 0]], [[2, 1, 0], [1, 0, 0], [2, 1, 0]],
                                       [[1, 0, 0], [1, 0, 0], [1, 0, 0]]]
    assert cf[0, [0, 2], 0].tolist() == [20.0, 5.0] and cols[0, 1, 0] == 0x7FC00000
    assert cf[1, [0, 2], 0].tolist() == [100.0, 5.0] and cols[1, 1, 0] == 0x7FC00000  # a group of two: its faster member
    assert (cols[2, :, 0] == 0x7FC00000).all()  # a rank alone in its group has no peer
    assert f[[0, 2, 4], 0, 0].tolist() == [2.0, 1.0, 0.5] and f[[1, 3], 0, 0].tolist() == [1.0, 0.5]
    assert recs[:, 0, 2].tolist() == [1, 1, 1, 1, 1, 0] and recs[3, 0, 3:5].tolist() == [1, 0]
    assert recs[5, :, 2:].tolist() == [[0] * 6] * 2 and (recs[5, :, :2] == 0x7FC00000).all()
    assert f[3, 1, 0] == np.float32(5.0 / 6.0) and f[4, 0, 7] == 1.0 * (1 - 0.5)


def test_restatement_guards_the_contents_of_the_group_array():
    rng = np.random.default_rng(5)
    R, K, S = 6, 3, 2
    T = _small_table(rng, R, K, S)
    g = _groups([0, 1, 0, 1, 0, 1])
    good = pace_group_scores_table(T, K, S, g.host, 2, 3, 0, R, 2, 2)
    bad = g.host.copy()
    bad[1] = 7          # rank 1: no such group
    bad[R + 1] = -3     # a member that is no rank: skipped (rank 2 leaves group 0's statistics)
    bad[2 * R + 2] = 99  # the last start word beyond R: clamped
    cols, recs, _ = pace_group_scores_table(T, K, S, bad, 2, 3, 0, R, 2, 2)
    assert (recs[1, :, 2:] == 0).all() and (recs[1, :, :2] == 0x7FC00000).all()
    assert np.array_equal(cols[1], good[0][1])
    assert (cols[0, :, 1] <= 2).all()
    # a stretch longer than max_group is cut; decreasing start words give an empty group
    cut = pace_group_scores_table(T, K, S, g.host, 2, 2, 0, R, 1, 1)[0]
    assert (cut[:, :, 1] <= 2).all()
    rev = g.host.copy()
    rev[2 * R : 2 * R + 3] = [5, 2, -4]
    assert (pace_group_scores_table(T, K, S, rev, 2, 3, 0, R, 1, 1)[0][:, :, 1] == 0).all()


@pytest.mark.parametrize("size,need", [(1, 2), (2, 2), (3, 3), (4, 4), (5, 4)])
def test_the_threshold_rule_at_group_sizes_one_to_five(size, need):
    """``max(min_peers, min(min_ranks, size))`` with the defaults 4 and 2."""
    assert threshold(4, 2, size) == need
    K, S = 1, 0
    T = np.zeros((size, 4), dtype=np.float32)
    T[:, 0] = np.arange(1, size + 1)
    g = _groups([0] * size)
    for present in range(size + 1):
        t = T.copy()
        t[present:, 0] = -1.0
        cols, recs, _ = pace_group_scores_table(t, K, S, g.host, 1, size, min_ranks=4, min_peers=2)
        referenced = cols[0, 0, 0] != 0x7FC00000
        assert cols[0, 0, 1] == present and referenced == (present >= need), (size, present)
        assert recs[0, 0, 2] == (1 if referenced else 0)


# ---- 2. the example's scenario ------------------------------------------------------------------------------------------------
def _load(rings, rows, med):
    for lr in range(med.shape[0]):
        for k, row in enumerate(rows.values()):
            rings.push_many(row, np.full(workers.SAMPLES, med[lr, k], dtype=np.float32), lr=lr)


@pytest.mark.parametrize("emulate_fused", [False, True])
@pytest.mark.parametrize("seed", workers.SEEDS)
@pytest.mark.parametrize("layout", sorted(workers.LAYOUTS))
def test_the_pipeline_scenario(layout, seed, emulate_fused):
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator

    be = PaceGroupOracleBackend(emulate_fused=emulate_fused)
    backend.set_backend(be)
    try:
        med = workers.scenario_medians(layout, seed)
        R, K = med.shape
        n = int(layout.partition(":")[2])
        named = {}
        for grouped in (False, True):
            gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=True, node_name="n", pace_scores=True,
                                  peer_groups=layout, pace_peer_groups=grouped)
            rings = be.make_rings(R, K, 256)
            rows = {name: rings.row_for(1, name) for name in workers.KERNEL_NAMES}
            for _ in range(2):  # the general path (_assemble), then the planned one
                _load(rings, rows, med)
                rep = gen.generate_report_from_rings(rings, {}, rows, local_ranks=R)
                rings.reset()
                named[grouped] = ranks_named(rep.identify_pace_stragglers())
                t = rep.pace_scores()
                json.dumps(t)
                if not grouped:
                    assert named[False] == workers.LAYOUTS[layout] and "groups" not in t
                    continue
                assert named[True] == [workers.SLOW_RANK]
                assert t["params"] == {"min_ranks": 4, "min_columns": 8, "min_effect": 0.03, "min_breadth": 0.9, "min_peers": 2,
                                       "peer_groups": True}
                assert t["groups"] == {g: list(range(g * n, g * n + n)) for g in range(R // n)}
                assert t["group_of"] == {r: r // n for r in range(R)} and t["unrated_ranks"] == []
                assert sorted(t["kernels"]) == sorted(rows) and t["section_columns"] == {}
                assert all(sorted(c) == list(range(R // n)) and all(x["ranks"] == n for x in c.values()) for c in t["kernels"].values())
                slow = t["ranks"][workers.SLOW_RANK]["gpu"]
                # 1 / 1.04 = 0.9615; the median of 120 quotients, each with about 1 % noise, lies well within 0.5 % of it
                assert 0.956 <= slow["pace"] <= 0.967 and slow["slower"] >= 118 and slow["columns"] == K
                for r in set(range(R)) - {workers.SLOW_RANK}:
                    gpu = t["ranks"][r]["gpu"]
                    assert 0.99 <= gpu["pace"] <= 1.005 and gpu["breadth"] < 0.9, (r, gpu)
            gen.close()
        assert be.pace_calls == 2 and be.pace_group_calls == 2
        assert be.pace_group_args == [(R, R // n, n, 0, R, 4, 2)] * 2
    finally:
        backend.set_backend(None)


def test_a_rank_alone_in_its_group_is_unrated_and_listed(cpu_backend):
    from nvrx_straggler import Statistic as S
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=True, node_name="n", pace_scores=True, pace_min_columns=1,
                          peer_groups=["solo"], pace_peer_groups=True)
    summ = {S.MIN: 1.0, S.MAX: 2.0, S.MED: 1.5, S.AVG: 1.5, S.STD: 0.1, S.NUM: 4}
    t = gen.generate_report({"sec": summ}, {"gemm": summ}).pace_scores()
    assert t["unrated_ranks"] == [0] and t["groups"] == {"solo": [0]} and t["group_of"] == {0: "solo"}
    assert t["ranks"][0]["gpu"]["columns"] == 0 and math.isnan(t["ranks"][0]["gpu"]["pace"]) and t["ranks"][0]["gpu"]["breadth"] is None
    assert t["kernels"]["gemm"]["solo"]["ranks"] == 1 and math.isnan(t["kernels"]["gemm"]["solo"]["center"])
    assert cpu_backend.pace_group_args == [(1, 1, 1, 0, 1, 1, 2)]
    gen.close()


# ---- 3. the option's values ------------------------------------------------------------------------------------------------
def test_option_values(cpu_backend, monkeypatch):
    from nvrx_straggler import Detector
    from nvrx_straggler.folded import FoldedJob  # noqa: F401  (its keyword is checked below by signature)
    from nvrx_straggler.reporting import ReportGenerator
    import inspect

    with pytest.raises(ValueError, match="pace_peer_groups needs pace_scores and peer_groups; pace_scores and peer_groups are not set"):
        ReportGenerator(["relative_perf_scores"], pace_peer_groups=True)
    with pytest.raises(ValueError, match="pace_peer_groups needs pace_scores and peer_groups; peer_groups is not set"):
        ReportGenerator(["relative_perf_scores"], pace_scores=True, pace_peer_groups=True)
    with pytest.raises(ValueError, match="pace_peer_groups needs pace_scores and peer_groups; pace_scores is not set"):
        ReportGenerator(["relative_perf_scores"], peer_groups="block:2", pace_peer_groups=True)
    gen = ReportGenerator(["relative_perf_scores"], pace_scores=True, peer_groups="block:2", pace_peer_groups=True)
    assert gen.pace_peer_groups is True
    assert ReportGenerator(["relative_perf_scores"], pace_scores=True, peer_groups="block:2").pace_peer_groups is False
    assert ReportGenerator(["relative_perf_scores"]).pace_peer_groups is False
    assert inspect.signature(FoldedJob.__init__).parameters["pace_peer_groups"].default is False
    with pytest.raises(ValueError, match="pace_peer_groups needs pace_scores and peer_groups"):
        Detector.initialize(node_name="n0", pace_peer_groups=True)
    assert not Detector.initialized
    # the environment variable is the Detector's default, read only when the argument is None
    for env, arg, want in (("1", None, True), ("1", False, False), ("0", None, False), ("", None, False), (None, True, True),
                           (None, None, False)):
        if env is None:
            monkeypatch.delenv("NVRX_PACE_PEER_GROUPS", raising=False)
        else:
            monkeypatch.setenv("NVRX_PACE_PEER_GROUPS", env)
        Detector.initialize(node_name="n0", pace_scores=True, peer_groups="mod:2", **({} if arg is None else {"pace_peer_groups": arg}))
        try:
            assert Detector.reporter.pace_peer_groups is want, (env, arg)
        finally:
            Detector.shutdown()
    monkeypatch.setenv("NVRX_PACE_PEER_GROUPS", "yes")
    with pytest.raises(ValueError, match="NVRX_PACE_PEER_GROUPS must be 0 or 1"):
        Detector.initialize(node_name="n0", pace_scores=True, peer_groups="mod:2")
    assert not Detector.initialized
    Detector.initialize(node_name="n0", pace_scores=True, peer_groups="mod:2", pace_peer_groups=False)  # (the argument wins)
    Detector.shutdown()
    monkeypatch.setenv("NVRX_PACE_PEER_GROUPS", "1")
    with pytest.raises(ValueError, match="pace_peer_groups needs pace_scores and peer_groups; pace_scores and peer_groups are not set"):
        Detector.initialize(node_name="n0")
    assert not Detector.initialized


def test_option_needs_a_backend_with_pace_group_score_and_labels_for_every_rank():
    from nvrx_straggler import Statistic as S
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator
    from pace_oracle_backend import PaceOracleBackend

    backend.set_backend(PaceOracleBackend())
    try:
        with pytest.raises(RuntimeError, match=r"no pace scores per peer group \(backend.pace_group_score\)"):
            ReportGenerator(["relative_perf_scores"], pace_scores=True, peer_groups="block:2", pace_peer_groups=True)
        ReportGenerator(["relative_perf_scores"], pace_scores=True, peer_groups="block:2")
    finally:
        backend.set_backend(None)
    backend.set_backend(PaceGroupOracleBackend())
    try:  # a label list whose length differs from R: peer's ValueError at the first report
        gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=True, node_name="n", pace_scores=True,
                              peer_groups=[0, 0, 1], pace_peer_groups=True)
        summ = {S.MIN: 1.0, S.MAX: 2.0, S.MED: 1.5, S.AVG: 1.5, S.STD: 0.1, S.NUM: 4}
        with pytest.raises(ValueError, match="peer_groups has 3 labels, the job has 1 logical ranks"):
            gen.generate_report({"sec": summ}, {"gemm": summ})
        gen.close()
    finally:
        backend.set_backend(None)


# ---- 4. off: nothing new is called, also with pace_scores and peer_groups both on ---------------------------------------------
@pytest.mark.parametrize("emulate_fused,asynchronous", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("both_on", [False, True])
def test_option_off_calls_nothing_new(emulate_fused, asynchronous, both_on):
    from nvrx_straggler import Detector
    from nvrx_straggler import Statistic as S
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator

    be = CountingPaceGroupBackend(emulate_fused=emulate_fused)
    backend.set_backend(be)
    options = dict(pace_scores=True, pace_min_ranks=1, peer_groups="block:1", peer_min_ranks=1) if both_on else {}
    try:
        gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=True, node_name="n",
                              asynchronous=asynchronous, **options)
        assert gen.pace_peer_groups is False
        summ = {S.MIN: 1.0, S.MAX: 2.0, S.MED: 1.5, S.AVG: 1.5, S.STD: 0.1, S.NUM: 4}

        def todays_shape(t):
            if not both_on:
                return t == {}
            return (sorted(t) == ["kernels", "params", "ranks", "section_columns"]
                    and t["params"] == {"min_ranks": 1, "min_columns": 8, "min_effect": 0.03, "min_breadth": 0.9}
                    and all(sorted(c) == ["above", "below", "center", "ranks"] for c in t["kernels"].values()))

        rep = gen.generate_report({"sec": summ}, {"k": summ})
        assert todays_shape(rep.pace_scores()) and todays_shape(pickle.loads(pickle.dumps(rep)).pace_scores())
        rings = be.make_rings(1, 8, 16)
        krow, srow = rings.row_for(1, "kern"), rings.row_for(0, "sec")
        for i in range(3):
            rings.push_many(krow, [1.0 + i, 2.0, 3.0])
            rings.push_many(srow, [5.0, 6.0])
            rep = gen.generate_report_from_rings(rings, {"sec": srow}, {"kern": krow})
            rings.reset()
            assert todays_shape(rep.pace_scores())
        assert gen._ring_plan is not None
        gen.close()
        Detector.initialize(scores_to_compute="all", gather_on_rank0=True, node_name="n0", asynchronous=asynchronous, **options)
        try:
            for t in range(3):
                for name, value in (("a", 2.0 + t), ("b", 4.0)):
                    with Detector.detection_section(name, profile_cuda=False):
                        pass
                    sec = Detector.custom_sections[name]
                    sec.cpu_elapsed_times.clear()
                    sec.cpu_elapsed_times.extend(np.full(5, value, dtype=np.float32))
                assert todays_shape(Detector.generate_report().pace_scores())
        finally:
            Detector.shutdown()
        assert be.pace_group_calls == 0 and (be.pace_calls > 0) == both_on
    finally:
        backend.set_backend(None)


# ---- 5. all attachment sites, behind robust and peer --------------------------------------------------------------------------
@pytest.mark.parametrize("emulate_fused,asynchronous", [(False, False), (True, False), (True, True)])
def test_all_three_attachment_sites(emulate_fused, asynchronous):
    from nvrx_straggler import Statistic as S
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator

    be = PaceGroupOracleBackend(emulate_fused=emulate_fused)
    backend.set_backend(be)
    try:
        order = []
        for name in ("robust_score", "peer_score", "pace_group_score"):
            def spy(*a, _name=name, _inner=getattr(be, name), **kw):
                order.append(_name)
                return _inner(*a, **kw)
            setattr(be, name, spy)
        gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=True, node_name="n",
                              asynchronous=asynchronous, pace_scores=True, robust_scores=True, peer_groups="block:1",
                              peer_min_ranks=1, pace_min_columns=1, pace_peer_groups=True)
        # (a) the dict-input report: _assemble
        summ = {S.MIN: 1.0, S.MAX: 2.0, S.MED: 1.5, S.AVG: 1.5, S.STD: 0.1, S.NUM: 4}
        t = gen.generate_report({"sec": summ}, {"gemm": summ}).pace_scores()
        assert order == ["robust_score", "peer_score", "pace_group_score"]
        assert t["kernels"] == {"gemm": {0: {"center": 1.5, "ranks": 1, "above": 0, "below": 0}}}
        assert t["section_columns"] == {"sec": {0: {"center": 1.5, "ranks": 1, "above": 0, "below": 0}}}
        assert t["ranks"][0]["gpu"] == {"pace": 1.0, "spread": 0.0, "columns": 1, "slower": 0, "faster": 0, "breadth": 0.0,
                                        "total_us": 6.0, "slower_us": 0.0, "excess_us": 0.0}
        assert t["params"]["min_ranks"] == 1 and t["params"]["min_peers"] == 1 and t["unrated_ranks"] == []
        # (b) ring reports: _assemble for the first, then the planned path -- stepwise, or one call through the rings
        rings = be.make_rings(1, 8, 16)
        kernel_rows = {"gemm": rings.row_for(1, "gemm")}
        section_rows = {"sec": rings.row_for(0, "sec")}
        before = be.pace_group_calls
        for w in range(4):
            v = np.arange(1, 12, dtype=np.float32) * (w + 1)
            rings.push_many(kernel_rows["gemm"], v)
            rings.push_many(section_rows["sec"], v[::-1] + 0.5)
            t = gen.generate_report_from_rings(rings, section_rows, kernel_rows).pace_scores()
            rings.reset()
            assert t["kernels"] == {"gemm": {0: {"center": 6.0 * (w + 1), "ranks": 1, "above": 0, "below": 0}}}
            assert t["section_columns"]["sec"][0]["center"] == 6.0 * (w + 1) + 0.5
            assert t["ranks"][0]["gpu"]["pace"] == 1.0 and t["ranks"][0]["gpu"]["total_us"] == float(np.float32(v.sum()))
        assert gen._ring_plan is not None and gen._ring_plan.fused == emulate_fused
        assert be.pace_group_calls - before == 4 and be.pace_group_args[-1] == (1, 1, 1, 0, 1, 1, 1)
        through_rings = be.pace_group_calls - order.count("pace_group_score")
        assert through_rings == (3 if emulate_fused else 0)
        assert be.pace_calls == 0  # the job-wide step is replaced, not run next to it
        gen.close()
    finally:
        backend.set_backend(None)


# ---- 6. no further collective; only where the rank holds a report, for the ranks it covers ---------------------------------
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("gather_on_rank0,emulate_fused", [(True, False), (False, False), (True, True)])
def test_the_option_adds_no_collective_and_covers_the_reports_ranks(world, gather_on_rank0, emulate_fused):
    kw = dict(gather_on_rank0=gather_on_rank0, emulate_fused=emulate_fused)
    on = run_ranks(workers.ring_reports_recorded, world, timeout=300, grouped=True, **kw)
    off = run_ranks(workers.ring_reports_recorded, world, timeout=300, grouped=False, **kw)
    G = (world + 1) // 2
    for r in range(world):
        assert on[r]["calls"] == off[r]["calls"], r
        holds = r == 0 or not gather_on_rank0
        assert off[r]["pace_group_calls"] == 0 and off[r]["pace_calls"] == (6 if holds else 0)
        assert on[r]["pace_group_calls"] == (6 if holds else 0) and on[r]["pace_calls"] == 0
        want = (world, G, 2, 0, world, 2, 2) if gather_on_rank0 else (world, G, 2, r, 1, 2, 2)
        assert all(a == want for a in on[r]["pace_group_args"]), on[r]["pace_group_args"]
        assert on[r]["fused"][0] is None and on[r]["fused"][-1] is emulate_fused  # the general path, then the plan
        for entry in on[r]["reports"]:
            if not holds:
                assert entry["pace"] is None
                continue
            t = entry["pace"]
            assert entry["pickled_same"]
            shown = list(range(world)) if gather_on_rank0 else [r]
            assert sorted(t["ranks"]) == shown and t["group_of"] == {x: x // 2 for x in shown}
            assert t["groups"] == {g: [x for x in range(world) if x // 2 == g] for g in range(G)}
            assert {"k0", "k1"} <= set(t["kernels"]) and "ncclDevKernel_z" not in t["kernels"]
            assert all(c[0]["ranks"] == 2 for n, c in t["kernels"].items() if n in ("k0", "k1"))
            assert {"s0", "s1"} <= set(t["section_columns"])
            # with three ranks the last one is alone in its group: unrated, not rated 1.0
            assert t["unrated_ranks"] == [x for x in shown if world == 3 and x == 2]


# ---- 7. lifetime and pickling -------------------------------------------------------------------------------------------------
def test_a_held_report_keeps_its_pace_scores_and_reports_travel(cpu_backend):
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=True, node_name="n", pace_scores=True,
                          peer_groups=["g"], peer_min_ranks=1, pace_peer_groups=True)
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
    handles = cpu_backend.pace_group_handles
    assert cpu_backend.pace_group_calls == 4 and all(h.reads == 0 for h in handles)  # generate_report reads nothing
    for w in (1, 0, 3, 2):  # a report held across the next two is still its own
        t = held[w].pace_scores()
        assert handles[w].reads == 1
        assert t["kernels"]["gemm"]["g"]["center"] == 6.0 * (w + 1) and t["section_columns"]["sec"]["g"]["center"] == 6.0 * (w + 1) + 0.5
        assert held[w].pace_scores() == t and handles[w].reads == 1
        for clone in (pickle.loads(pickle.dumps(held[w])), copy.deepcopy(held[w])):
            assert json.dumps(clone.pace_scores()) == json.dumps(t)
            assert clone.identify_pace_stragglers() == held[w].identify_pace_stragglers()
            assert isinstance(clone.__dict__["_pace"], dict)  # materialised
    t = held[0].pace_scores()
    t["kernels"].clear()
    t["groups"]["g"].clear()
    t["ranks"][0]["gpu"].clear()
    again = held[0].pace_scores()
    assert again["kernels"] and again["groups"] == {"g": [0]} and again["ranks"][0]["gpu"]


# ---- 8. the lane declines, as for pace scores --------------------------------------------------------------------------------
def test_lane_declines_while_the_option_is_on():
    from types import SimpleNamespace

    from nvrx_straggler import straggler

    reporter = SimpleNamespace(_ring_plan=SimpleNamespace(fused=True, ws=None), world_size=1, _exchanged=lambda: True,
                               _direct=None, asynchronous=False, kernel_attribution=0, tail_q_ppm=0, pace_scores=True,
                               peer_groups=("block", 2), pace_peer_groups=True)
    rings = SimpleNamespace(lib=SimpleNamespace(nvrx_window_report=object()))
    det = SimpleNamespace(_rings=rings, reporter=reporter, _cupti_manager=None, _pending_region_switch=None)
    assert straggler._Lane.build(det) is None


# ---- 9. the Lightning callback ------------------------------------------------------------------------------------------------
def test_callback_warns_of_a_rank_off_its_groups_pace_and_never_halts_for_it(monkeypatch):
    import callback_script
    import nvrx_straggler
    from nvidia_resiliency_ext.ptl_resiliency import StragglerDetectionCallback
    from nvrx_straggler.reporting import Report

    healthy = callback_script._scores(8)
    base = {k: v for k, v in callback_script.reports(8)[1].items() if not k.startswith("gpu_")}
    sequence = [None, {6: 0.961}, None, {}, {6: 0.95, 2: 0.9}, {6: 0.985}]

    def pace_of(slow):
        def gpu(r):
            pace = slow.get(r, 1.0)
            slower = 120 if r in slow else 55
            return {"pace": pace, "spread": 0.007, "columns": 120, "slower": slower, "faster": 120 - slower,
                    "breadth": slower / 120, "total_us": 1e6, "slower_us": 1e6 * slower / 120, "excess_us": 1e6 * (1 - pace)}
        none = {"pace": float("nan"), "spread": float("nan"), "columns": 0, "slower": 0, "faster": 0, "breadth": None}
        return {"ranks": {r: {"gpu": gpu(r), "sections": dict(none)} for r in range(8)}, "kernels": {}, "section_columns": {},
                "params": {"min_ranks": 4, "min_columns": 8, "min_effect": 0.03, "min_breadth": 0.9, "min_peers": 2,
                           "peer_groups": True},
                "groups": {0: [0, 1, 2, 3], 1: [4, 5, 6, 7]}, "group_of": {r: r // 4 for r in range(8)}, "unrated_ranks": []}

    peer = {"groups": {0: [0, 1, 2, 3], 1: [4, 5, 6, 7]}, "group_of": {r: r // 4 for r in range(8)}, "min_ranks": 2,
            "gpu_relative": {r: 1.0 for r in range(8)}, "section_relative": {}, "section_floor": {}, "section_fastest": {},
            "kernel_floor": {}, "ranks_with_data": {}, "unrated_ranks": []}

    def scripted(n_ranks):
        return [None if e is None else dict(base, gpu_relative_perf_scores=healthy, gpu_individual_perf_scores=healthy,
                                            pace=pace_of(e)) for e in sequence]

    def make_report(pace=None, **fields):
        rep = Report(**fields)
        rep.__dict__["_pace"] = pace
        rep.__dict__["_peer"] = peer
        return rep

    monkeypatch.setattr(callback_script, "reports", scripted)
    monkeypatch.setitem(callback_script.CONFIGS, "off_group_pace", dict(callback_script.CONFIGS["print2_log_stop"], warn_if_off_pace=True,
                                                                        peer_groups="block:4", pace_peer_groups=True))
    got = callback_script.drive(StragglerDetectionCallback, nvrx_straggler, make_report,
                                ("off_group_pace", "off_group_pace", 8, 0, False, False, False))
    assert got["initialize_calls"] == [dict(scores_to_compute=["relative_perf_scores", "individual_perf_scores"],
                                            gather_on_rank0=True, profiling_interval=1, report_time_interval=1.0,
                                            peer_groups="block:4", pace_scores=True, pace_peer_groups=True)]
    its = got["iterations"]
    warnings = [[m for level, m in it["records"] if level == "WARNING"] for it in its]
    assert [len(w) for w in warnings] == [0, 1, 0, 0, 1, 0]  # one warning per report that names anybody
    assert warnings[1] == ["STRAGGLER DETECTION WARNING: Some GPUs are off their peer group's pace, a little slower than their "
                           "group's median in nearly all of their kernels (degraded card?): rank 6 (pace 0.961, slower in 120 of "
                           "120 kernels, excess_us=39000)"]
    assert "rank 2 (pace 0.900" in warnings[4][0] and "rank 6 (pace 0.950" in warnings[4][0]
    assert [it["should_stop"] for it in its] == [False] * len(sequence) and all(it["exit"] is None for it in its)  # stop_if_detected=True

    # the default, given or not: the initialize call and the transcript of today
    monkeypatch.undo()
    monkeypatch.setitem(callback_script.CONFIGS, "explicit_off", dict(callback_script.CONFIGS["print2_log_stop"], pace_peer_groups=False))
    plain = callback_script.drive(StragglerDetectionCallback, nvrx_straggler, Report, callback_script.SCENARIOS[0])
    given = callback_script.drive(StragglerDetectionCallback, nvrx_straggler, Report,
                                  ("rank0_8ranks", "explicit_off", 8, 0, False, False, False))
    assert json.dumps(dict(given, config=None), sort_keys=True) == json.dumps(dict(plain, config=None), sort_keys=True)
    assert given["initialize_calls"] == [dict(scores_to_compute=["relative_perf_scores", "individual_perf_scores"],
                                              gather_on_rank0=True, profiling_interval=1, report_time_interval=1.0)]
    with pytest.raises(ValueError, match="pace_peer_groups needs warn_if_off_pace"):
        StragglerDetectionCallback(**dict(callback_script.CONFIGS["print2_log_stop"], peer_groups="block:4", pace_peer_groups=True))
    with pytest.raises(ValueError, match="pace_peer_groups needs peer_groups"):
        StragglerDetectionCallback(**dict(callback_script.CONFIGS["print2_log_stop"], warn_if_off_pace=True, pace_peer_groups=True))


# ---- 10. header, bindings and macros agree ---------------------------------------------------------------------------------------
def test_bindings_follow_the_header():
    import os
    import re

    from nvrx_straggler import _native

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nvrx_straggler.h")).read()
    symbols = {name: args for name, _, args in _native.SYMBOLS}
    for name in ("nvrx_pace_group_score", "nvrx_report_pace_group"):
        m = re.search(r"int " + name + r"\(([^;]*)\);", header)
        assert m, name
        assert len(m.group(1).split(",")) == len(symbols[name]), name
    assert "#define NVRX_PACE_GROUP_WORDS(G, n_ranks, K, S) (4 * (size_t)(G) * ((size_t)(K) + (S)) + 16 * (size_t)(n_ranks))" in header
    assert _native.pace_group_words(3, 5, 7, 2) == 4 * 3 * 9 + 16 * 5
    assert _native.pace_group_words(1, 5, 7, 2) == _native.pace_words(5, 7, 2)
