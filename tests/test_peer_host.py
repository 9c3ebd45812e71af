"""Peer-group scores, host side, on the CPU checker backend (tests/peer_oracle_backend.py): the restatement on a table worked
out by hand, the option's plumbing through ReportGenerator / Detector / FoldedJob / Report / the Lightning callback, the
motivating two-stage job, that the option adds no collective on gloo ranks, the step together with other follow-ups, lifetime
and pickling, and the argument checks of the two C entry points (callable without a device).

Bounds: column records and section scores are compared exactly (an actual value; one f64 quotient rounded to f32); GPU slots
of the checker are the restatement's own sequential sums, compared exactly."""
import copy
import json
import math
import os
import pickle
import re
import subprocess

import numpy as np
import pytest

import peer_workers
from mp_util import run_ranks
from peer_oracle_backend import (CountingPeerBackend, PeerOracleBackend, STAGE_SLOW_RANK, peer_columns, peer_group_arrays,
                                 peer_scores_table, stage_medians)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECTION = "training_step.forward"


@pytest.fixture
def cpu_backend():
    from nvrx_straggler import backend

    be = PeerOracleBackend()
    backend.set_backend(be)
    try:
        yield be
    finally:
        backend.set_backend(None)


# ---- 1. the restatement itself, on a table worked out by hand -----------------------------------------------------------------
def test_restatement_on_a_hand_worked_table():
    from nvrx_straggler import _native
    from nvrx_straggler.backend import PeerGroups

    K, S = 1, 2
    arrays, names = peer_group_arrays(["a", "b", "a", "a", "b", "c"])
    assert names == ["a", "b", "c"]
    assert arrays.tolist() == [0, 1, 0, 0, 1, 2] + [0, 2, 3, 1, 4, 5] + [0, 3, 5, 6]
    product = PeerGroups(["a", "b", "a", "a", "b", "c"])  # the product resolves the same array
    assert product.host.tolist() == arrays.tolist() and product.labels == ("a", "b", "c") and product.G == 3
    T = np.full((6, _native.table_len(K, S)), -1.0, dtype=np.float32)
    T[:, 0] = [10.0, 20.0, 10.0, 12.0, 25.0, 7.0]  # a: 10 10 12, a tie -> rank 0; b: 20 25; c: alone
    T[:, 1] = [5.0, -1.0, 4.0, np.nan, 8.0, 3.0]   # a: rank 3 absent -> 5 4; b: one present member
    T[:, 2] = [-1.0, 6.0, -1.0, -1.0, 9.0, -1.0]   # a: nobody has it; b: 6 9
    T[:, 2 * (K + S)] = [2.0, 1.0, 1.0, 1.0, 1.0, 1.0]  # kernel weights
    cols, sc = peer_scores_table(T, K, S, arrays, 3, min_ranks=2)
    nan = 0x7FC00000
    f = lambda x: int(np.float32(x).view(np.uint32))  # noqa: E731
    m1 = 0xFFFFFFFF
    assert cols[0].tolist() == [[f(10.0), 3, 0, 3], [f(4.0), 2, 2, 3], [nan, 0, m1, 3]]
    assert cols[1].tolist() == [[f(20.0), 2, 1, 2], [nan, 1, m1, 2], [f(6.0), 2, 1, 2]]
    assert cols[2].tolist() == [[nan, 1, m1, 1], [nan, 1, m1, 1], [nan, 0, m1, 1]]  # a singleton has no peer
    assert sc[0, 0] == 1.0 and sc[0, 1] == np.float32(4.0 / 5.0) and math.isnan(sc[0, 2])
    assert sc[2, 0] == 1.0 and sc[2, 1] == 1.0 and math.isnan(sc[2, 2])
    assert sc[3, 0] == np.float32(10.0 / 12.0) and math.isnan(sc[3, 1]) and math.isnan(sc[3, 2])  # absent in section 0
    assert sc[1, 0] == 1.0 and math.isnan(sc[1, 1]) and sc[1, 2] == 1.0
    assert sc[4, 0] == np.float32(20.0 / 25.0) and math.isnan(sc[4, 1]) and sc[4, 2] == np.float32(6.0 / 9.0)
    assert np.isnan(sc[5]).all()  # unrated, not rated 1.0
    # min_ranks = 1: the singleton and the one-member pair are their own reference; the all-absent pairs still have none
    cols1, sc1 = peer_scores_table(T, K, S, arrays, 3, min_ranks=1)
    assert cols1[2].tolist() == [[f(7.0), 1, 5, 1], [f(3.0), 1, 5, 1], [nan, 0, m1, 1]]
    assert cols1[1, 1].tolist() == [f(8.0), 1, 4, 2] and cols1[0, 2].tolist() == [nan, 0, m1, 3]
    assert sc1[5, 0] == 1.0 and sc1[5, 1] == 1.0 and math.isnan(sc1[5, 2]) and sc1[4, 1] == 1.0
    # a sub-range is the slice of the whole
    colsp, scp = peer_scores_table(T, K, S, arrays, 3, first_rank=2, n_ranks=3, min_ranks=2)
    assert np.array_equal(colsp, cols) and np.array_equal(scp.view(np.uint32), sc[2:5].view(np.uint32))
    # min_ranks is not clamped to the group's size
    assert np.isnan(peer_columns(T, K, S, arrays, 3, 4).view(np.float32)[:, :, 0]).all()
    assert _native.peer_words(3, 6, K, S) == 4 * 3 * 3 + 6 * 3 and _native.PEER_MAX_GROUPS == 4096


# ---- 2. the option's values ---------------------------------------------------------------------------------------------------
def test_option_values_and_refusals(cpu_backend, monkeypatch):
    from nvrx_straggler import Detector
    from nvrx_straggler.backend import PeerGroups
    from nvrx_straggler.reporting import ReportGenerator

    rel = ["relative_perf_scores"]
    assert ReportGenerator(rel).peer_groups is None
    gen = ReportGenerator(rel, peer_groups="block:4")
    assert gen.peer_groups == ("block", 4) and gen.peer_min_ranks == 2
    assert PeerGroups.resolve(gen.peer_groups, 8).group.tolist() == [0, 0, 0, 0, 1, 1, 1, 1]
    gen = ReportGenerator(rel, peer_groups="mod:3", peer_min_ranks=1)
    assert gen.peer_min_ranks == 1 and PeerGroups.resolve(gen.peer_groups, 7).group.tolist() == [0, 1, 2, 0, 1, 2, 0]
    for labels in (["x", "y", "x"], ("x", "y", "x"), np.array(["x", "y", "x"])):
        groups = PeerGroups.resolve(ReportGenerator(rel, peer_groups=labels).peer_groups, 3)
        assert groups.labels == ("x", "y") and groups.members(0) == [0, 2] and groups.members(1) == [1]
    groups = PeerGroups.resolve(ReportGenerator(rel, peer_groups=np.array([7, 7, 3])).peer_groups, 3)
    assert groups.labels == (7, 3) and all(type(x) is int for x in groups.labels)  # first appearance by ascending rank
    for bad in ("block", "block:", "block:x", "stage:2", "mod:-1", "block:1.5", ""):
        with pytest.raises(ValueError, match="peer_groups"):
            ReportGenerator(rel, peer_groups=bad)
    for bad in ("block:0", "mod:0"):
        with pytest.raises(ValueError, match="at least 1"):
            ReportGenerator(rel, peer_groups=bad)
    for bad in (lambda r: r // 4, {0: "a"}, 4, 2.5, {1, 2}, range(4)):
        with pytest.raises(TypeError, match="peer_groups"):
            ReportGenerator(rel, peer_groups=bad)
    for bad in ([0, 1.5], [0, None], ["a", ("b",)], [True, False]):
        with pytest.raises(TypeError, match="labels must be int or str"):
            ReportGenerator(rel, peer_groups=bad)
    with pytest.raises(ValueError, match="peer_groups"):
        ReportGenerator(rel, peer_groups=[])
    with pytest.raises(ValueError, match="peer_groups"):
        ReportGenerator(rel, peer_groups=np.zeros((2, 2), dtype=np.int64))
    for bad in (0, -1, 2.5, "2", None, True):
        with pytest.raises(ValueError, match="peer_min_ranks"):
            ReportGenerator(rel, peer_groups="block:2", peer_min_ranks=bad)
    ReportGenerator(rel, peer_min_ranks=0)  # (not looked at while the option is off)
    with pytest.raises(ValueError, match="peer_groups.*relative_perf_scores"):
        ReportGenerator(["individual_perf_scores"], peer_groups="block:2")
    with pytest.raises(ValueError, match="peer_groups.*relative_perf_scores"):
        Detector.initialize(scores_to_compute=["individual_perf_scores"], peer_groups="block:2")
    assert not Detector.initialized
    # the environment variables are the Detector's defaults, read only when the argument is None
    for value, want in (("block:4", ("block", 4)), ("mod:2", ("mod", 2)), ("0,0,1,1", (0, 0, 1, 1)), (" 3 , 3 ", (3, 3))):
        monkeypatch.setenv("NVRX_PEER_GROUPS", value)
        Detector.initialize(node_name="n0")
        try:
            assert Detector.reporter.peer_groups == want and Detector.reporter.peer_min_ranks == 2
        finally:
            Detector.shutdown()
    monkeypatch.setenv("NVRX_PEER_MIN_RANKS", "3")
    Detector.initialize(node_name="n0")
    try:
        assert Detector.reporter.peer_min_ranks == 3
    finally:
        Detector.shutdown()
    Detector.initialize(node_name="n0", peer_groups="mod:5", peer_min_ranks=1)
    try:
        assert Detector.reporter.peer_groups == ("mod", 5) and Detector.reporter.peer_min_ranks == 1
    finally:
        Detector.shutdown()
    monkeypatch.setenv("NVRX_PEER_MIN_RANKS", "two")
    with pytest.raises(ValueError, match="NVRX_PEER_MIN_RANKS"):
        Detector.initialize(node_name="n0")
    monkeypatch.delenv("NVRX_PEER_MIN_RANKS")
    monkeypatch.setenv("NVRX_PEER_GROUPS", "a,b")
    with pytest.raises(ValueError, match="NVRX_PEER_GROUPS"):
        Detector.initialize(node_name="n0")
    monkeypatch.setenv("NVRX_PEER_GROUPS", "")
    Detector.initialize(node_name="n0")
    try:
        assert Detector.reporter.peer_groups is None
    finally:
        Detector.shutdown()
    monkeypatch.delenv("NVRX_PEER_GROUPS")
    Detector.initialize(node_name="n0")
    try:
        assert Detector.reporter.peer_groups is None
    finally:
        Detector.shutdown()


def test_length_mismatch_and_too_many_groups_are_refused_at_the_first_report(cpu_backend):
    from nvrx_straggler import Statistic as S
    from nvrx_straggler.backend import PeerGroups
    from nvrx_straggler.reporting import ReportGenerator

    summ = {S.MIN: 1.0, S.MAX: 2.0, S.MED: 1.5, S.AVG: 1.5, S.STD: 0.1, S.NUM: 4}
    gen = ReportGenerator(["relative_perf_scores"], node_name="n", peer_groups=[0, 0, 1])
    with pytest.raises(ValueError, match=r"3 labels.*1 logical ranks"):
        gen.generate_report({"sec": summ}, {"k": summ})
    gen = ReportGenerator(["relative_perf_scores"], node_name="n", peer_groups=["only"], peer_min_ranks=1)
    t = gen.generate_report({"sec": summ}, {"k": summ}).peer_scores()
    assert t["groups"] == {"only": [0]} and t["section_relative"] == {"sec": {0: 1.0}} and t["gpu_relative"] == {0: 1.0}
    with pytest.raises(ValueError, match="4097 groups, at most 4096"):
        PeerGroups.resolve(tuple(range(4097)), 4097)
    assert PeerGroups.resolve(tuple(range(4096)), 4096).G == 4096
    with pytest.raises(ValueError, match="4097 groups"):
        PeerGroups.resolve(ReportGenerator(["relative_perf_scores"], peer_groups="block:1").peer_groups, 4097)


def test_option_needs_a_backend_with_peer_score():
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator
    from slack_oracle_backend import SlackOracleBackend

    backend.set_backend(SlackOracleBackend())
    try:
        with pytest.raises(RuntimeError, match="no peer-group scores"):
            ReportGenerator(["relative_perf_scores"], peer_groups="block:2")
        ReportGenerator(["relative_perf_scores"])
    finally:
        backend.set_backend(None)


# ---- 3. off by default: nothing is called -------------------------------------------------------------------------------------
@pytest.mark.parametrize("emulate_fused,asynchronous", [(False, False), (True, False), (True, True)])
def test_default_is_off_and_calls_nothing(emulate_fused, asynchronous):
    from nvrx_straggler import Detector
    from nvrx_straggler import Statistic as S
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator

    be = CountingPeerBackend(emulate_fused=emulate_fused)
    backend.set_backend(be)
    try:
        gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=True, node_name="n",
                              asynchronous=asynchronous)
        assert gen.peer_groups is None
        summ = {S.MIN: 1.0, S.MAX: 2.0, S.MED: 1.5, S.AVG: 1.5, S.STD: 0.1, S.NUM: 4}
        rep = gen.generate_report({"sec": summ}, {"k": summ})
        assert rep.peer_scores() == {} and pickle.loads(pickle.dumps(rep)).peer_scores() == {}
        assert rep.identify_peer_stragglers() == {"straggler_gpus_relative": set(), "straggler_sections_relative": {}}
        rings = be.make_rings(1, 8, 16)
        krow, srow = rings.row_for(1, "kern"), rings.row_for(0, "sec")
        kernel_rows, section_rows = {"kern": krow}, {"sec": srow}
        for i in range(3):
            rings.push_many(krow, [1.0 + i, 2.0, 3.0])
            rings.push_many(srow, [5.0, 6.0])
            rep = gen.generate_report_from_rings(rings, section_rows, kernel_rows)
            rings.reset()
            assert rep.peer_scores() == {}
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
                assert Detector.generate_report().peer_scores() == {}
        finally:
            Detector.shutdown()
        assert be.peer_calls == 0
    finally:
        backend.set_backend(None)


# ---- 4. the motivating table, end to end -------------------------------------------------------------------------------------
def _load(rings, names, med):
    rows = {n: rings.row_for(0, n) for n in names}
    for lr in range(med.shape[0]):
        for s, n in enumerate(names):
            rings.push_many(rows[n], np.full(5, med[lr, s], dtype=np.float32), lr=lr)
    return rows


@pytest.mark.parametrize("emulate_fused,asynchronous", [(False, False), (True, False), (True, True)])
def test_two_stages_name_four_ranks_by_the_job_and_one_by_its_peers(emulate_fused, asynchronous):
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator

    be = PeerOracleBackend(emulate_fused=emulate_fused)
    backend.set_backend(be)
    try:
        med = stage_medians().astype(np.float32)
        gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=True, node_name="n", peer_groups="block:4",
                              asynchronous=asynchronous)
        rings = be.make_rings(8, 4, 16)
        rows = _load(rings, [SECTION], med)
        for i in range(3):  # the general path, then the planned one
            if i:
                _load(rings, [SECTION], med)
            rep = gen.generate_report_from_rings(rings, rows, {}, local_ranks=8)
            rings.reset()
            job = rep.section_relative_perf_scores[SECTION]
            assert [round(job[r], 3) for r in range(8)] == [1.0] * 4 + [0.667, 0.667, 0.476, 0.667]
            assert peer_workers.flagged(rep.identify_stragglers()) == [4, 5, 6, 7]
            assert peer_workers.flagged(rep.identify_peer_stragglers()) == [STAGE_SLOW_RANK]
            t = rep.peer_scores()
            json.dumps({k: v for k, v in t.items() if k not in ("groups", "group_of")})
            assert t["groups"] == {0: [0, 1, 2, 3], 1: [4, 5, 6, 7]} and t["group_of"] == {r: r // 4 for r in range(8)}
            assert t["min_ranks"] == 2 and t["unrated_ranks"] == [] and t["kernel_floor"] == {}
            assert all(math.isnan(v) for v in t["gpu_relative"].values()) and sorted(t["gpu_relative"]) == list(range(8))
            peer = t["section_relative"][SECTION]
            assert [round(peer[r], 3) for r in range(8)] == [1.0] * 6 + [0.714, 1.0]
            assert t["section_floor"] == {SECTION: {0: 1000.0, 1: 1500.0}}
            assert t["section_fastest"] == {SECTION: {0: 0, 1: 4}}  # (ties: the lowest rank)
            assert t["ranks_with_data"] == {SECTION: {0: 4, 1: 4}}
        assert be.peer_calls == 3 and all(a == (8, 2, 0, 8, 2) for a in be.peer_args)
        gen.close()
    finally:
        backend.set_backend(None)


def test_a_rank_alone_in_its_group_is_unrated(cpu_backend):
    from nvrx_straggler.reporting import ReportGenerator

    med = stage_medians().astype(np.float32)
    gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=True, node_name="n",
                          peer_groups=["s0"] * 4 + ["s1"] * 3 + ["loss"])
    rings = cpu_backend.make_rings(8, 4, 16)
    rep = gen.generate_report_from_rings(rings, _load(rings, [SECTION], med), {}, local_ranks=8)
    t = rep.peer_scores()
    assert t["unrated_ranks"] == [7] and math.isnan(t["section_relative"][SECTION][7])
    assert t["groups"] == {"s0": [0, 1, 2, 3], "s1": [4, 5, 6], "loss": [7]} and t["group_of"][7] == "loss"
    assert t["section_floor"] == {SECTION: {"s0": 1000.0, "s1": 1500.0}} and t["ranks_with_data"] == {SECTION: {"s0": 4, "s1": 3, "loss": 1}}
    assert peer_workers.flagged(rep.identify_peer_stragglers()) == [STAGE_SLOW_RANK]
    gen.close()


# ---- 5. one group, min_ranks = 1: the report's own relative section scores ----------------------------------------------------
@pytest.mark.parametrize("emulate_fused", [False, True])
def test_one_group_and_one_rank_minimum_give_the_reports_relative_section_scores(emulate_fused):
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator

    be = PeerOracleBackend(emulate_fused=emulate_fused)
    backend.set_backend(be)
    try:
        rng = np.random.default_rng(3)
        names = [f"sec{s}" for s in range(6)]
        gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=True, node_name="n", peer_groups="block:8",
                              peer_min_ranks=1)
        rings = be.make_rings(8, 8, 16)
        for i in range(2):
            med = rng.lognormal(5.0, 0.4, (8, 6)).astype(np.float32)
            rows = _load(rings, names, med)
            rep = gen.generate_report_from_rings(rings, rows, {}, local_ranks=8)
            rings.reset()
            t = rep.peer_scores()
            assert t["groups"] == {0: list(range(8))}
            assert t["section_relative"] == {n: dict(v) for n, v in rep.section_relative_perf_scores.items()}
            assert sorted(t["section_relative"]) == names
        gen.close()
    finally:
        backend.set_backend(None)


# ---- 6. no further collective; the right ranks; folded jobs -------------------------------------------------------------------
@pytest.mark.parametrize("world,local_ranks", [(2, 1), (3, 1), (2, 2)])
@pytest.mark.parametrize("gather_on_rank0", [True, False])
def test_the_option_adds_no_collective_and_covers_the_reports_ranks(world, local_ranks, gather_on_rank0):
    kw = dict(timeout=300, gather_on_rank0=gather_on_rank0, local_ranks=local_ranks)
    on = run_ranks(peer_workers.ring_reports_recorded, world, peer_groups="mod:2", **kw)
    off = run_ranks(peer_workers.ring_reports_recorded, world, peer_groups=None, **kw)
    R = world * local_ranks
    group = [q % 2 for q in range(R)]  # (with two logical ranks per process the groups cut through every process)
    for r in range(world):
        assert on[r]["calls"] == off[r]["calls"], r
        assert off[r]["peer_calls"] == 0 and all(e["peer"] in ({}, None) for e in off[r]["reports"])
        holds = r == 0 or not gather_on_rank0
        assert on[r]["peer_calls"] == (6 if holds else 0), on[r]["peer_calls"]
        want = (0, R) if gather_on_rank0 else (r * local_ranks, local_ranks)
        assert all(a == (R, 2, *want, 1) for a in on[r]["peer_args"]), on[r]["peer_args"]
    for i in range(6):
        med = {key: [m for q in range(world) for m in on[q]["reports"][i]["medians"].get(key, [None] * local_ranks)]
               for key in ("section:s0", "section:s1")}
        for r in range(world):
            entry = on[r]["reports"][i]
            if gather_on_rank0 and r != 0:
                assert entry["peer"] is None
                continue
            t = entry["peer"]
            assert entry["pickled_same"]
            covered = list(range(R)) if gather_on_rank0 else list(range(r * local_ranks, (r + 1) * local_ranks))
            assert sorted(t["gpu_relative"]) == covered and t["group_of"] == {q: group[q] for q in covered}
            assert t["groups"] == {g: [q for q in range(R) if group[q] == g] for g in (0, 1)}  # every rank of the job
            assert t["min_ranks"] == 1 and t["unrated_ranks"] == []
            for key, meds in med.items():
                name = key.split(":")[1]
                meds = np.array(meds, dtype=np.float32)
                for q in covered:
                    peers = [p for p in range(R) if group[p] == group[q]]
                    floor = meds[peers].min()
                    assert t["section_relative"][name][q] == float(np.float32(np.float64(floor) / np.float64(meds[q]))), (i, r, name, q)
                    assert t["section_floor"][name][group[q]] == float(floor)
                    assert t["section_fastest"][name][group[q]] == peers[int(np.argmin(meds[peers]))]
                    assert t["ranks_with_data"][name][group[q]] == len(peers)
            assert "ncclDevKernel_z" not in t["kernel_floor"] and "k0" in t["kernel_floor"]


# ---- 7. together with other follow-ups ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("emulate_fused,asynchronous", [(False, False), (True, False), (True, True)])
def test_together_with_attribution_robust_scores_and_a_row_family(emulate_fused, asynchronous):
    res = peer_workers.ring_reports_recorded(0, 1, True, peer_groups="block:1", emulate_fused=emulate_fused,
                                             asynchronous=asynchronous, kernel_attribution=2, robust_scores=True,
                                             robust_min_ranks=1, tail_quantile=0.9)
    from nvrx_straggler import backend

    backend.set_backend(None)
    assert res["peer_calls"] == 6
    for entry in res["reports"]:
        assert entry["pickled_same"] and entry["explained"] == ["individual", "relative"]
        assert "gpu_relative" in entry["tails"] and "gpu_z" in entry["robust"]
        t = entry["peer"]
        assert t["gpu_relative"] == {0: 1.0} and t["groups"] == {0: [0]} and t["min_ranks"] == 1
        assert all(v == {0: 1.0} for v in t["section_relative"].values()) and "s0" in t["section_relative"]


# ---- 8. lifetime and pickling ------------------------------------------------------------------------------------------------
def test_a_held_report_keeps_its_peer_scores_and_reports_travel(cpu_backend):
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=True, node_name="n",
                          peer_groups=["a", "a"], peer_min_ranks=2)
    rings = cpu_backend.make_rings(2, 8, 16)
    kernel_rows = {n: rings.row_for(1, n) for n in ("gemm", "ncclDevKernel_y")}
    section_rows = {"sec": rings.row_for(0, "sec")}
    held = []
    for w in range(4):
        v = np.arange(1, 12, dtype=np.float32) * (w + 1)
        for lr in range(2):
            rings.push_many(kernel_rows["gemm"], v * (lr + 1), lr=lr)
            rings.push_many(kernel_rows["ncclDevKernel_y"], v * 100, lr=lr)
            rings.push_many(section_rows["sec"], (v[::-1] + 0.5) * (2 - lr), lr=lr)
        held.append(gen.generate_report_from_rings(rings, section_rows, kernel_rows, local_ranks=2))
        rings.reset()
    assert gen._ring_plan is not None and cpu_backend.peer_calls == 4
    assert all(h.reads == 0 for h in cpu_backend.peer_handles)  # generate_report reads nothing
    for w in (3, 2, 1, 0):
        t = held[w].peer_scores()
        assert cpu_backend.peer_handles[w].reads == 1
        assert t["kernel_floor"] == {"gemm": {"a": 6.0 * (w + 1)}} and t["section_floor"] == {"sec": {"a": 6.0 * (w + 1) + 0.5}}
        assert t["gpu_relative"] == {0: 1.0, 1: 0.5} and t["section_relative"] == {"sec": {0: 0.5, 1: 1.0}}
        assert t["section_fastest"] == {"sec": {"a": 1}} and t["ranks_with_data"] == {"gemm": {"a": 2}, "sec": {"a": 2}}
        assert held[w].peer_scores() == t and cpu_backend.peer_handles[w].reads == 1
        for clone in (pickle.loads(pickle.dumps(held[w])), copy.deepcopy(held[w])):
            assert json.dumps(clone.peer_scores()) == json.dumps(t)
            assert clone.identify_peer_stragglers() == held[w].identify_peer_stragglers()
        assert peer_workers.flagged(held[w].identify_peer_stragglers()) == [0, 1]
    t = held[0].peer_scores()
    t["kernel_floor"].clear()
    t["section_relative"]["sec"].clear()
    t["groups"]["a"].clear()
    t["unrated_ranks"].append(9)
    again = held[0].peer_scores()
    assert again["kernel_floor"] and again["section_relative"]["sec"] and again["groups"] == {"a": [0, 1]} and again["unrated_ranks"] == []


# ---- 9. thresholds -----------------------------------------------------------------------------------------------------------
def test_thresholds_are_strict_and_nan_is_never_flagged():
    from nvrx_straggler.reporting import Report

    rep = Report({}, {}, {}, {}, {0: "a", 1: "b", 2: "c"}, {}, {}, 0.0, True, 0)
    rep.__dict__["_peer"] = {"gpu_relative": {0: 0.75, 1: 0.7499, 2: float("nan")},
                             "section_relative": {"s": {0: 0.0, 1: 9.0, 2: float("nan")}, "t": {0: 0.75, 1: 0.8, 2: 1.0}}}
    found = rep.identify_peer_stragglers()
    assert {s.rank for s in found["straggler_gpus_relative"]} == {1}
    assert {n: {s.rank for s in v} for n, v in found["straggler_sections_relative"].items()} == {"s": {0}}
    found = rep.identify_peer_stragglers(gpu_rel_threshold=0.5, section_rel_threshold=0.9)
    assert found["straggler_gpus_relative"] == set()
    assert {n: {s.rank for s in v} for n, v in found["straggler_sections_relative"].items()} == {"s": {0}, "t": {0, 1}}


# ---- 10. the lane declines ---------------------------------------------------------------------------------------------------
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

    def det(groups):
        reporter = SimpleNamespace(_ring_plan=SimpleNamespace(fused=True, ws=None), world_size=1, _exchanged=lambda: True,
                                   _direct=None, asynchronous=False, kernel_attribution=0, tail_q_ppm=0, robust_scores=False,
                                   peer_groups=groups)
        rings = SimpleNamespace(lib=SimpleNamespace(nvrx_window_report=object()))
        return SimpleNamespace(_rings=rings, reporter=reporter, _cupti_manager=Manager(), _pending_region_switch=None)

    with pytest.raises(Reached):
        straggler._Lane.build(det(None))
    assert straggler._Lane.build(det(("block", 4))) is None
    assert straggler._Lane.build(det((0, 0, 1, 1))) is None


# ---- 11. the Lightning callback ----------------------------------------------------------------------------------------------
def test_callback_halts_for_the_peer_straggler_only(monkeypatch):
    import sys

    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    try:
        import callback_script
    finally:
        sys.path.pop(0)
    import nvrx_straggler
    from nvidia_resiliency_ext.ptl_resiliency import StragglerDetectionCallback
    from nvrx_straggler.reporting import Report

    healthy = callback_script._scores(8)
    base = {k: v for k, v in callback_script.reports(8)[1].items() if not k.startswith("gpu_")}
    job = {r: x for r, x in enumerate([1.0] * 4 + [0.667, 0.667, 0.476, 0.667])}
    peers = {r: x for r, x in enumerate([1.0] * 6 + [0.714, 1.0])}
    healthy_peers = {r: 1.0 for r in range(8)}
    healthy_peers[7] = float("nan")

    def scripted(n_ranks):
        stage = dict(base, gpu_relative_perf_scores=job, gpu_individual_perf_scores=healthy)
        return [None, dict(stage, peer={"gpu_relative": healthy_peers, "section_relative": {}, "unrated_ranks": [7]}),
                dict(stage, peer={"gpu_relative": healthy_peers, "section_relative": {}, "unrated_ranks": [7]}),
                dict(stage, peer={"gpu_relative": peers, "section_relative": {}, "unrated_ranks": []})]

    def make_report(peer=None, **fields):
        rep = Report(**fields)
        rep.__dict__["_peer"] = peer
        return rep

    monkeypatch.setattr(callback_script, "reports", scripted)
    config = dict(callback_script.CONFIGS["print2_log_stop"], gpu_relative_perf_threshold=0.75)
    monkeypatch.setitem(callback_script.CONFIGS, "stages", config)
    monkeypatch.setitem(callback_script.CONFIGS, "stages_peer", dict(config, peer_groups="block:4"))
    today = callback_script.drive(StragglerDetectionCallback, nvrx_straggler, make_report, ("today", "stages", 8, 0, False, False, False))
    assert today["initialize_calls"] == [dict(scores_to_compute=["relative_perf_scores", "individual_perf_scores"],
                                              gather_on_rank0=True, profiling_interval=1, report_time_interval=1.0)]
    first = [m for level, m in today["iterations"][1]["records"] if level == "WARNING"]
    assert len(first) == 1 and "worse relative performance" in first[0]
    assert [int(x) for x in re.findall(r"rank=(\d+)", first[0])] == [4, 5, 6, 7]
    assert today["iterations"][1]["should_stop"]  # a healthy job is stopped at its first report

    got = callback_script.drive(StragglerDetectionCallback, nvrx_straggler, make_report, ("peer", "stages_peer", 8, 0, False, False, False))
    assert got["initialize_calls"] == [dict(scores_to_compute=["relative_perf_scores", "individual_perf_scores"],
                                            gather_on_rank0=True, profiling_interval=1, report_time_interval=1.0,
                                            peer_groups="block:4")]
    its = got["iterations"]
    warnings = [[m for level, m in it["records"] if level == "WARNING"] for it in its]
    assert [len(w) for w in warnings] == [0, 0, 0, 1]
    assert warnings[3][0].startswith("STRAGGLER DETECTION WARNING: Some GPUs have worse performance than their peer group. Affected ranks:")
    assert [int(x) for x in re.findall(r"rank=(\d+)", warnings[3][0])] == [STAGE_SLOW_RANK]
    assert [it["should_stop"] for it in its] == [False, False, False, True]
    unrated = [[m for level, m in it["records"] if level == "INFO" and "not rated" in m] for it in its]
    assert [len(u) for u in unrated] == [0, 1, 0, 0] and "[7]" in unrated[1][0]  # once, at the first report

    with pytest.raises(ValueError, match="peer_groups cannot be combined with min_consecutive_reports"):
        StragglerDetectionCallback(**dict(config, peer_groups="block:4", min_consecutive_reports=2))
    with pytest.raises(ValueError, match="peer_groups needs calc_relative_gpu_perf"):
        StragglerDetectionCallback(**dict(callback_script.CONFIGS["print3_indiv_only_log"], peer_groups="block:4"))
    StragglerDetectionCallback(**dict(config, min_consecutive_reports=2))  # (without the option: as before)


# ---- 12. header, bindings and macros agree; the C entry points check their arguments before any device is touched --------------
def test_entry_points_check_their_arguments_without_a_device():
    import ctypes

    from nvrx_straggler import _native

    lib = _native.load()
    assert {"nvrx_peer_score", "nvrx_report_peer"} <= {name for name, _, _ in _native.SYMBOLS}
    assert lib.nvrx_abi_version() == 2
    with open(os.path.join(REPO, "include", "nvrx_straggler.h")) as f:
        header = " ".join(f.read().split())
    assert ("int nvrx_peer_score(const float *d_table, int R, int K, int S, const int32_t *d_groups, int G, int first_rank, "
            "int n_ranks, int min_ranks, void *d_out, void *stream);") in header
    assert ("int nvrx_report_peer(nvrx_ctx *ctx, const nvrx_report_desc *desc, const int32_t *d_groups, int G, int first_rank, "
            "int n_ranks, int min_ranks, void *d_out);") in header
    assert "#define NVRX_PEER_MAX_GROUPS 4096" in header
    assert "#define NVRX_PEER_WORDS(G, n_ranks, K, S) (4 * (size_t)(G) * ((size_t)(K) + (S)) + (size_t)(n_ranks) * (1 + (size_t)(S)))" in header
    assert _native.peer_words(8, 1024, 64, 64) == 4 * 8 * 128 + 1024 * 65
    fake = ctypes.c_void_p(4096)

    def score(table=fake, R=8, K=8, S=2, groups=fake, G=2, first=0, n=8, min_ranks=2, out=fake):
        return lib.nvrx_peer_score(table, R, K, S, groups, G, first, n, min_ranks, out, None)

    assert score(R=0) == _native.ERR_INVALID and b"shape" in lib.nvrx_last_error()
    assert score(R=-1) == _native.ERR_INVALID and score(K=-1) == _native.ERR_INVALID and score(S=-1) == _native.ERR_INVALID
    assert score(R=65537, n=1) == _native.ERR_RANGE and b"ranks" in lib.nvrx_last_error()
    assert score(K=70000) == _native.ERR_RANGE and score(S=70000) == _native.ERR_RANGE
    assert score(first=7, n=2) == _native.ERR_RANGE and b"outside the table" in lib.nvrx_last_error()
    assert score(first=-1) == _native.ERR_RANGE and score(n=0) == _native.ERR_RANGE and score(n=9) == _native.ERR_RANGE
    assert score(min_ranks=0) == _native.ERR_RANGE and b"min_ranks" in lib.nvrx_last_error()
    assert score(min_ranks=-3) == _native.ERR_RANGE
    assert score(G=0) == _native.ERR_INVALID and b"groups" in lib.nvrx_last_error()
    assert score(G=-2) == _native.ERR_INVALID
    assert score(G=9) == _native.ERR_RANGE and b"groups" in lib.nvrx_last_error()
    assert score(R=65536, G=4097) == _native.ERR_RANGE and b"at most 4096" in lib.nvrx_last_error()
    assert score(table=None) == _native.ERR_INVALID and score(out=None) == _native.ERR_INVALID
    assert score(groups=None) == _native.ERR_INVALID and b"null" in lib.nvrx_last_error()
    assert score(out=ctypes.c_void_p(4100)) == _native.ERR_INVALID and b"aligned" in lib.nvrx_last_error()

    desc = _native.ReportDesc()
    desc.R, desc.K, desc.S = 8, 8, 2

    def report(ctx=fake, d=ctypes.byref(desc), groups=fake, G=2, first=0, n=8, min_ranks=2, out=fake):
        return lib.nvrx_report_peer(ctx, d, groups, G, first, n, min_ranks, out)

    assert report(ctx=None) == _native.ERR_INVALID and report(d=None) == _native.ERR_INVALID
    assert report(first=1) == _native.ERR_RANGE and report(n=0) == _native.ERR_RANGE
    assert report(min_ranks=0) == _native.ERR_RANGE
    assert report(G=0) == _native.ERR_INVALID and report(G=9) == _native.ERR_RANGE
    assert report(groups=None) == _native.ERR_INVALID
    assert report(out=None) == _native.ERR_INVALID and report(out=ctypes.c_void_p(4104)) == _native.ERR_INVALID


def test_the_args_check_program_runs_clean():
    """``make peer-args-check``: both entries with invalid arguments only, host code under ASan + UBSan, a stand-alone program."""
    out = subprocess.run(["make", "-C", os.path.join(REPO, "nvidia-resiliency-ext_amd", "csrc"), "peer-args-check"],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "peer_args_check: 0 failure(s)" in out.stdout
