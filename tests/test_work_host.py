"""Work groups on a box without a GPU: the NumPy restatement against hand-written expectations, the options, the host side of
a report on the CPU checker backend, and the entry points' argument checks (which touch no device)."""
import copy
import ctypes
import functools
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import work_workers
from mp_util import run_ranks
from peer_workers import flagged
from work_cases import CASES, readme_scenario
from work_oracle_backend import CountingWorkBackend, WorkOracleBackend, groups_of, work_block, work_layout, work_pair

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = ["relative_perf_scores"]


@pytest.fixture
def cpu_backend():
    from nvrx_straggler import backend

    be = WorkOracleBackend()
    backend.set_backend(be)
    try:
        yield be
    finally:
        backend.set_backend(None)


@functools.lru_cache(maxsize=None)
def _block(name):
    c = CASES[name]
    return work_block(c["T"], c["K"], c["S"], c["count_tol"], c["max_unlike_ppm"])


def _alike(adj, a, b):
    return bool((int(adj[a, b // 64]) >> (b % 64)) & 1)


# ---- 1. the restatement against what the rule says, written by hand -----------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_restatement_gives_the_hand_written_expectations(name):
    c, b = CASES[name], _block(name)
    R = c["T"].shape[0]
    rec = b["ranks"]
    root = rec[:, 0].view(np.int32)
    assert groups_of(root) == c["groups"]
    for g, members in c["groups"].items():
        assert g == min(members) and all(rec[r, 1] == len(members) for r in members)
    assert b["job"].tolist()[:3] == [len(c["groups"]), sum(len(m) == 1 for m in c["groups"].values()),
                                     max(len(m) for m in c["groups"].values())]
    for r, (near, unlike, either) in c.get("nearest", {}).items():
        assert (int(rec[r, 3].view(np.int32)), int(rec[r, 4]), int(rec[r, 5])) == (near, unlike, either), r
    if "sig" in c:
        assert np.array_equal(b["sig"].view(np.uint32), c["sig"].view(np.uint32))
    assert all(_alike(b["adj"], x, y) and _alike(b["adj"], y, x) for x, y in c.get("alike", []))
    assert not any(_alike(b["adj"], x, y) or _alike(b["adj"], y, x) for x, y in c.get("not_alike", []))
    if "loose" in c:
        assert [r for r in range(R) if rec[r, 2] + 1 < rec[r, 1]] == c["loose"]
    # the block's own invariants: the diagonal, no bit at or beyond R, symmetry, the degree, a nearest that is a partial record
    T = work_layout(R, c["K"], c["S"])["T"]
    for a in range(R):
        assert _alike(b["adj"], a, a)
        assert sum(bin(int(w)).count("1") for w in b["adj"][a]) == rec[a, 2] + 1
        assert (int(b["adj"][a, T - 1]) >> ((R - 1) % 64 + 1)) == 0
        near = int(rec[a, 3].view(np.int32))
        if near >= 0:
            assert b["part"][a, near // 64].tolist() == [rec[a, 4], rec[a, 5], near, 0]
    if R <= 130:
        for a in range(R):
            for o in range(a + 1, R):
                assert _alike(b["adj"], a, o) == _alike(b["adj"], o, a)
    assert b["words"].size == work_layout(R, c["K"], c["S"])["words"]


def test_the_pair_rule_one_column_at_a_time():
    """``work_pair`` -- the rule as a loop over columns -- against the row-at-a-time form the block is built from."""
    for name in ("readme_two_stages", "edge_values", "chain_of_12", "count_boundary", "nearest_ties"):
        c, b = CASES[name], _block(name)
        R = c["T"].shape[0]
        for a in range(R):
            for o in range(R):
                if a != o:
                    assert work_pair(b["sig"][a], b["sig"][o], c["count_tol"]) == (b["unlike"][a, o], b["either"][a, o]), (name, a, o)


def test_the_readme_scenario_in_numbers():
    """The slow rank differs from its stage's peers in 0 of 114 columns and from the other stage in 120 of 124; with the call
    counts as the only difference the groups come out the same."""
    b = _block("readme_two_stages")
    assert b["unlike"][6].tolist() == [120] * 4 + [0] * 4 and b["either"][6].tolist() == [124] * 4 + [114, 114, 0, 114]
    b = _block("readme_counts_only")
    assert b["unlike"][6].tolist() == [100] * 4 + [0] * 4 and b["either"][6].tolist() == [104] * 4 + [104, 104, 0, 104]
    T, K, S = readme_scenario(noise=0.0)
    assert groups_of(work_block(T, K, S)["root"]) == CASES["readme_two_stages"]["groups"]


# ---- 2. options ------------------------------------------------------------------------------------------------------------
def test_option_values_and_refusals(cpu_backend, monkeypatch):
    from nvrx_straggler import Detector
    from nvrx_straggler.reporting import ReportGenerator, _peer_spec
    from nvrx_straggler.straggler import _peer_groups_from_env

    gen = ReportGenerator(REL)
    assert gen.work_groups is False and gen.peer_groups is None
    gen = ReportGenerator(REL, work_groups=True)
    assert gen.work_groups and (gen.work_count_tol, gen.work_max_unlike, gen.work_max_unlike_ppm) == (0.25, 0.1, 100000)
    gen = ReportGenerator(REL, peer_groups="auto", work_count_tol=0, work_max_unlike=0.05)
    assert gen.peer_groups == "auto" and gen.work_groups and gen.work_max_unlike_ppm == 50000 and gen.work_count_tol == 0.0
    assert _peer_spec("auto") == "auto" and _peer_groups_from_env(" auto ") == "auto"
    for bad in (-0.1, 16.5, float("nan"), "x", None, True):
        with pytest.raises(ValueError, match="work_count_tol"):
            ReportGenerator(REL, work_groups=True, work_count_tol=bad)
    for bad in (-0.1, 1.5, float("nan"), "x", True):
        with pytest.raises(ValueError, match="work_max_unlike"):
            ReportGenerator(REL, work_groups=True, work_max_unlike=bad)
    ReportGenerator(REL, work_count_tol=99)  # (off: the step's parameters are not looked at)
    with pytest.raises(ValueError, match="work_groups needs relative_perf_scores"):
        ReportGenerator(["individual_perf_scores"], work_groups=True)
    with pytest.raises(ValueError, match="peer_groups needs relative_perf_scores"):
        ReportGenerator(["individual_perf_scores"], peer_groups="auto")
    with pytest.raises(ValueError, match="node_groups='auto': only peer_groups are inferred"):
        ReportGenerator(REL, node_scores=True, node_groups="auto")
    with pytest.raises(ValueError, match="must be 'block:N'"):
        ReportGenerator(REL, peer_groups="automatic")
    ReportGenerator(REL, peer_groups="auto", pace_scores=True, pace_peer_groups=True)  # (auto counts as peer groups)

    def initialized(**kw):
        Detector.initialize(scores_to_compute="all", gather_on_rank0=True, node_name="n", **kw)
        try:
            r = Detector.reporter
            return r.peer_groups, r.work_groups, getattr(r, "work_count_tol", None), getattr(r, "work_max_unlike_ppm", None)
        finally:
            Detector.shutdown()

    assert initialized() == (None, False, None, None)
    assert initialized(work_groups=True) == (None, True, 0.25, 100000)
    assert initialized(peer_groups="auto", work_max_unlike=0.2) == ("auto", True, 0.25, 200000)
    monkeypatch.setenv("NVRX_WORK_GROUPS", "1")
    monkeypatch.setenv("NVRX_WORK_COUNT_TOL", "0.5")
    monkeypatch.setenv("NVRX_WORK_MAX_UNLIKE", "0.02")
    assert initialized() == (None, True, 0.5, 20000)
    assert initialized(work_groups=False) == (None, False, None, None)
    assert initialized(work_count_tol=1.0) == (None, True, 1.0, 20000)
    monkeypatch.setenv("NVRX_WORK_GROUPS", "0")
    monkeypatch.setenv("NVRX_PEER_GROUPS", "auto")
    assert initialized() == ("auto", True, 0.5, 20000)
    assert initialized(peer_groups="block:2") == (("block", 2), False, None, None)
    monkeypatch.setenv("NVRX_WORK_COUNT_TOL", "much")
    with pytest.raises(ValueError, match="NVRX_WORK_COUNT_TOL must be a number"):
        initialized()
    monkeypatch.delenv("NVRX_WORK_COUNT_TOL")
    monkeypatch.setenv("NVRX_WORK_GROUPS", "yes")
    with pytest.raises(ValueError, match="NVRX_WORK_GROUPS must be 0 or 1"):
        initialized()
    monkeypatch.setenv("NVRX_WORK_GROUPS", "0")
    monkeypatch.setenv("NVRX_NODE_SCORES", "1")
    monkeypatch.setenv("NVRX_NODE_GROUPS", "auto")
    with pytest.raises(ValueError, match="only peer_groups are inferred"):
        initialized()


def test_option_needs_a_backend_with_work_groups():
    from node_oracle_backend import NodeOracleBackend
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator

    backend.set_backend(NodeOracleBackend())
    try:
        with pytest.raises(RuntimeError, match="work_groups: the active backend .* has no work groups"):
            ReportGenerator(REL, work_groups=True)
        with pytest.raises(RuntimeError, match="peer_groups='auto': the active backend"):
            ReportGenerator(REL, peer_groups="auto")
        ReportGenerator(REL, peer_groups="block:2")
    finally:
        backend.set_backend(None)


def test_the_callback_hands_auto_through_and_is_unchanged_otherwise(monkeypatch):
    from nvidia_resiliency_ext.ptl_resiliency import StragglerDetectionCallback
    from nvidia_resiliency_ext.ptl_resiliency import straggler_det_callback as mod

    seen = []
    monkeypatch.setattr(mod.straggler.Detector, "initialize", classmethod(lambda cls, **kw: seen.append(kw)))
    monkeypatch.setattr(mod.straggler.Detector, "wrap_callables", classmethod(lambda cls, **kw: None))

    class Strategy:
        def training_step(self):
            pass

    trainer = type("Trainer", (), {"strategy": Strategy()})()
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    try:
        import callback_script
    finally:
        sys.path.pop(0)
    common = dict(callback_script.CONFIGS["print2_log_stop"], gpu_relative_perf_threshold=0.75)
    for groups in ("auto", "block:4", None):
        StragglerDetectionCallback(**common, **({} if groups is None else {"peer_groups": groups})).setup(trainer, None, "fit")
    assert seen[0]["peer_groups"] == "auto" and seen[1]["peer_groups"] == "block:4" and "peer_groups" not in seen[2]
    assert {k: v for k, v in seen[0].items() if k != "peer_groups"} == seen[2]
    assert not any(k.startswith("work_") for kw in seen for k in kw)


# ---- 3. reports on the checker backend ---------------------------------------------------------------------------------------
def _load_two_stages(rings, section_rows, kernel_rows, swap=()):
    for lr in range(8):
        stage = lr // 4 if lr not in swap else 1 - lr // 4
        sec, kernels = work_workers.stage_window(lr, len(section_rows), stage)
        for s, row in enumerate(section_rows.values()):
            rings.push_many(row, sec[s], lr=lr)
        for name, values in kernels.items():
            rings.push_many(kernel_rows[name], values, lr=lr)


@pytest.mark.parametrize("emulate_fused,asynchronous", [(False, False), (True, False), (True, True)])
def test_auto_names_the_slow_rank_alone_and_equals_explicit_labels(emulate_fused, asynchronous):
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator

    be = WorkOracleBackend(emulate_fused=emulate_fused)
    backend.set_backend(be)
    try:
        gens = {spec: ReportGenerator(REL, gather_on_rank0=True, node_name="n", peer_groups=spec, asynchronous=asynchronous,
                                      work_groups=True) for spec in ("auto", "block:4")}
        out = {}
        for spec, gen in gens.items():
            rings = be.make_rings(8, 20, 64)
            section_rows = {f"sec{s}": rings.row_for(0, f"sec{s}") for s in range(2)}
            kernel_rows = {k: rings.row_for(1, k) for k in work_workers.KERNELS}
            for i in range(3):  # the general path, then the planned one
                _load_two_stages(rings, section_rows, kernel_rows)
                rep = gen.generate_report_from_rings(rings, section_rows, kernel_rows, local_ranks=8)
                rings.reset()
                w = rep.work_groups()
                assert w["groups"] == {0: [0, 1, 2, 3], 4: [4, 5, 6, 7]} and w["group_of"] == {r: 4 * (r // 4) for r in range(8)}
                assert w["singletons"] == [] and w["ranks_with_data"] == 8
                assert w["params"] == {"count_tol": 0.25, "max_unlike": 0.1, "max_unlike_ppm": 100000}
                assert w["ranks"][6] == {"size": 4, "degree": 3, "loose": False, "nearest": 4, "nearest_unlike": 0,
                                         "nearest_columns": 12, "kernels": 10, "sections": 2}
                assert w["ranks"][0]["nearest"] == 1 and w["ranks"][3]["nearest"] == 0
                assert ("label_conflicts" in w) == (spec != "auto") and w.get("label_conflicts", {}) == {}
                json.dumps({k: v for k, v in w.items() if k not in ("groups", "group_of", "ranks")})
                assert flagged(rep.identify_stragglers()) == [4, 5, 6, 7]
                assert flagged(rep.identify_peer_stragglers()) == [work_workers.SLOW_RANK]
                out.setdefault(spec, []).append(rep.peer_scores())
            gen.close()
        for a, t in zip(out["auto"], out["block:4"]):
            assert a["groups"] == {0: [0, 1, 2, 3], 4: [4, 5, 6, 7]} and t["groups"] == {0: [0, 1, 2, 3], 1: [4, 5, 6, 7]}
            assert repr(a["gpu_relative"]) == repr(t["gpu_relative"]) and repr(a["section_relative"]) == repr(t["section_relative"])
        assert be.work_calls == 6 and all(a == (8, len(work_workers.KERNELS), 2, 0.25, 100000) for a in be.work_args)
        assert gens["auto"]._peer_resolved.labels == (0, 4)
    finally:
        backend.set_backend(None)


def test_auto_keeps_its_groups_object_while_the_roots_stay_and_follows_them_when_they_move(cpu_backend):
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(REL, gather_on_rank0=True, node_name="n", peer_groups="auto")
    rings = cpu_backend.make_rings(8, 20, 64)
    section_rows = {"sec": rings.row_for(0, "sec")}
    kernel_rows = {k: rings.row_for(1, k) for k in work_workers.KERNELS}
    seen = []
    for swap in ((), (), (2, 5), (2, 5), ()):
        _load_two_stages(rings, section_rows, kernel_rows, swap)
        rep = gen.generate_report_from_rings(rings, section_rows, kernel_rows, local_ranks=8)
        rings.reset()
        seen.append((gen._peer_resolved, rep.peer_scores()["groups"]))
    assert seen[0][0] is seen[1][0] and seen[2][0] is seen[3][0] and seen[1][0] is not seen[2][0] and seen[4][0] is not seen[3][0]
    assert seen[0][1] == {0: [0, 1, 2, 3], 4: [4, 5, 6, 7]} == seen[4][1] and seen[2][1] == {0: [0, 1, 3, 5], 2: [2, 4, 6, 7]}
    gen.close()


def test_label_conflicts_name_the_user_groups_that_the_work_splits(cpu_backend):
    from nvrx_straggler.reporting import ReportGenerator

    labels = ["a", "a", "a", "b", "b", "b", "b", "c"]  # rank 3 is in the wrong group; "c" is a part of stage 1
    gen = ReportGenerator(REL, gather_on_rank0=True, node_name="n", peer_groups=labels, work_groups=True)
    rings = cpu_backend.make_rings(8, 20, 64)
    section_rows = {"sec": rings.row_for(0, "sec")}
    kernel_rows = {k: rings.row_for(1, k) for k in work_workers.KERNELS}
    _load_two_stages(rings, section_rows, kernel_rows)
    w = gen.generate_report_from_rings(rings, section_rows, kernel_rows, local_ranks=8).work_groups()
    assert w["label_conflicts"] == {"b": {0: [3], 4: [4, 5, 6]}}  # ("a" and "c" lie within one inferred group each)
    w["label_conflicts"]["b"][0].append(9)
    gen.close()


def test_more_ranks_than_the_step_takes_are_refused_at_the_first_report(cpu_backend):
    from nvrx_straggler import _native
    from nvrx_straggler.reporting import ReportGenerator

    R = _native.WORK_MAX_RANKS + 1
    rings = cpu_backend.make_rings(R, 2, 4)
    rows = {"sec": rings.row_for(0, "sec")}
    for option, kw in (("peer_groups='auto'", {"peer_groups": "auto"}), ("work_groups", {"work_groups": True})):
        gen = ReportGenerator(REL, gather_on_rank0=True, node_name="n", **kw)
        before = (cpu_backend.work_calls, len(getattr(cpu_backend, "score_args", ())))
        with pytest.raises(ValueError, match=f"{option}: the job has 4097 logical ranks.*at most 4096.*peer_groups labels"):
            gen.generate_report_from_rings(rings, rows, {}, local_ranks=R)
        assert (cpu_backend.work_calls, len(getattr(cpu_backend, "score_args", ()))) == before  # nothing was launched
        gen.close()
    gen = ReportGenerator(REL, gather_on_rank0=True, node_name="n", peer_groups=f"block:{R}")  # labels: no such limit
    gen.close()


@pytest.mark.parametrize("emulate_fused,asynchronous", [(False, False), (True, False), (True, True)])
def test_default_is_off_and_a_report_makes_the_calls_it_made_before(emulate_fused, asynchronous):
    """With the option off nothing of the step is called (its methods raise); with it on, the backend and rings calls of three
    reports are those of the option off plus the step's own."""
    from nvrx_straggler import Statistic as S
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator

    def calls(be_cls, **kw):
        be = be_cls(emulate_fused=emulate_fused)
        log = []

        class Logged:
            def __init__(self, inner, prefix):
                object.__setattr__(self, "_inner", inner)
                object.__setattr__(self, "_prefix", prefix)

            def __getattr__(self, name):
                value = getattr(self._inner, name)
                if callable(value) and not name.startswith("_"):
                    def call(*a, **k):
                        log.append(self._prefix + name)
                        return value(*a, **k)
                    return call
                return value

            def __setattr__(self, name, value):
                setattr(self._inner, name, value)

        backend.set_backend(Logged(be, "backend."))
        try:
            gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=True, node_name="n",
                                  asynchronous=asynchronous, **kw)
            summ = {S.MIN: 1.0, S.MAX: 2.0, S.MED: 1.5, S.AVG: 1.5, S.STD: 0.1, S.NUM: 4}
            rep = gen.generate_report({"sec": summ}, {"k": summ})
            assert (rep.work_groups() == {}) == (not kw) and pickle.loads(pickle.dumps(rep)).work_groups() == rep.work_groups()
            rings = Logged(be.make_rings(1, 8, 16), "rings.")
            krow, srow = rings.row_for(1, "kern"), rings.row_for(0, "sec")
            kernel_rows, section_rows = {"kern": krow}, {"sec": srow}
            for i in range(3):
                rings.push_many(krow, [1.0 + i, 2.0, 3.0])
                rings.push_many(srow, [5.0, 6.0])
                rep = gen.generate_report_from_rings(rings, section_rows, kernel_rows)
                rings.reset()
                assert (rep.work_groups() == {}) == (not kw)
            assert gen._ring_plan is not None
            gen.close()
            return log, be.work_calls
        finally:
            backend.set_backend(None)

    off, off_calls = calls(CountingWorkBackend)
    on, on_calls = calls(WorkOracleBackend, work_groups=True)
    step = {"backend.work_groups", "rings.report_work"}
    assert off_calls == 0 and on_calls == 4 and not step & set(off)
    assert [name for name in on if name not in step] == off
    assert sorted(set(on) - set(off)) == (["backend.work_groups", "rings.report_work"] if emulate_fused else ["backend.work_groups"])


# ---- 4. no further collective; every rank infers the same groups --------------------------------------------------------------
@pytest.mark.parametrize("world,local_ranks", [(2, 1), (3, 1), (2, 2)])
@pytest.mark.parametrize("gather_on_rank0", [True, False])
def test_the_option_adds_no_collective_and_every_rank_infers_the_same_groups(world, local_ranks, gather_on_rank0):
    kw = dict(timeout=300, gather_on_rank0=gather_on_rank0, local_ranks=local_ranks)
    # (a name that only one process has yet -- the worker's s_new and k_new -- makes the ranks of a parity differ in at most 2
    # of 8 columns, and the two parities differ in at least 6 of 11: 0.34 lies between; lognormal samples: the counts are left out)
    on = run_ranks(work_workers.ring_reports_recorded, world, peer_groups="auto", peer_min_ranks=1, work_max_unlike=0.34,
                   work_count_tol=4.0, **kw)
    off = run_ranks(work_workers.ring_reports_recorded, world, **kw)
    R = world * local_ranks
    want = {g: [q for q in range(R) if q % 2 == g] for g in range(min(2, R))}
    for r in range(world):
        assert on[r]["calls"] == off[r]["calls"], r
        assert off[r]["work_calls"] == 0 and all(e["work"] in ({}, None) for e in off[r]["reports"])
        holds = r == 0 or not gather_on_rank0
        assert on[r]["work_calls"] == (6 if holds else 0), on[r]["work_calls"]
        for i, entry in enumerate(on[r]["reports"]):
            if not holds:
                assert entry["work"] is None
                continue
            w = entry["work"]
            covered = list(range(R)) if gather_on_rank0 else list(range(r * local_ranks, (r + 1) * local_ranks))
            assert w["groups"] == want and sorted(w["group_of"]) == covered == sorted(w["ranks"]), (r, i, w["groups"])
            assert entry["pickled_same"] and entry["peer"]["groups"] == want and sorted(entry["peer"]["gpu_relative"]) == covered


# ---- 5. lifetime and pickling ------------------------------------------------------------------------------------------------
def test_a_held_report_keeps_its_work_groups_and_reports_travel(cpu_backend):
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(REL, gather_on_rank0=True, node_name="n", work_groups=True)
    rings = cpu_backend.make_rings(8, 20, 64)
    section_rows = {"sec": rings.row_for(0, "sec")}
    kernel_rows = {k: rings.row_for(1, k) for k in work_workers.KERNELS}
    held = []
    for swap in ((), (2, 5), (), (2, 5)):
        _load_two_stages(rings, section_rows, kernel_rows, swap)
        held.append(gen.generate_report_from_rings(rings, section_rows, kernel_rows, local_ranks=8))
        rings.reset()
    assert gen._ring_plan is not None and cpu_backend.work_calls == 4
    assert all(h.reads == 0 for h in cpu_backend.work_handles)  # generate_report reads nothing
    for i in (3, 2, 1, 0):
        w = held[i].work_groups()
        assert cpu_backend.work_handles[i].reads == 1
        assert w["groups"] == ({0: [0, 1, 3, 5], 2: [2, 4, 6, 7]} if i % 2 else {0: [0, 1, 2, 3], 4: [4, 5, 6, 7]})
        assert held[i].work_groups() == w and cpu_backend.work_handles[i].reads == 1
        for clone in (pickle.loads(pickle.dumps(held[i])), copy.deepcopy(held[i])):
            assert repr(clone.work_groups()) == repr(w)
    w = held[0].work_groups()
    w["groups"][0].clear()
    w["ranks"][0]["size"] = 99
    w["singletons"].append(7)
    again = held[0].work_groups()
    assert again["groups"][0] == [0, 1, 2, 3] and again["ranks"][0]["size"] == 4 and again["singletons"] == []
    gen.close()


# ---- 6. the lane declines ----------------------------------------------------------------------------------------------------
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

    def det(**options):
        reporter = SimpleNamespace(_ring_plan=SimpleNamespace(fused=True, ws=None), world_size=1, _exchanged=lambda: True,
                                   _direct=None, asynchronous=False, kernel_attribution=0, tail_q_ppm=0, robust_scores=False,
                                   peer_groups=None, **options)
        rings = SimpleNamespace(lib=SimpleNamespace(nvrx_window_report=object()))
        return SimpleNamespace(_rings=rings, reporter=reporter, _cupti_manager=Manager(), _pending_region_switch=None)

    with pytest.raises(Reached):
        straggler._Lane.build(det())
    with pytest.raises(Reached):
        straggler._Lane.build(det(work_groups=False))
    assert straggler._Lane.build(det(work_groups=True)) is None


# ---- 7. header, bindings and layout agree; the C entry points check their arguments before any device is touched ---------------
def test_entry_points_check_their_arguments_without_a_device():
    from nvrx_straggler import _native

    lib = _native.load()
    assert {"nvrx_work_groups", "nvrx_report_work", "nvrx_work_words"} <= {name for name, _, _ in _native.SYMBOLS}
    assert lib.nvrx_abi_version() == 2
    with open(os.path.join(REPO, "include", "nvrx_straggler.h")) as f:
        header = " ".join(f.read().split())
    assert ("int nvrx_work_groups(const float *d_table, int R, int K, int S, float count_tol, int max_unlike_ppm, void *d_out, "
            "void *stream);") in header
    assert "int nvrx_report_work(nvrx_ctx *ctx, const nvrx_report_desc *desc, float count_tol, int max_unlike_ppm, void *d_out);" in header
    assert "int nvrx_work_words(int R, int K, int S);" in header and "#define NVRX_WORK_MAX_RANKS 4096" in header
    assert _native.WORK_MAX_RANKS == 4096
    for R, K, S in ((1, 0, 0), (1, 2, 1), (8, 12, 4), (64, 5, 1), (65, 3, 0), (130, 66, 4), (1100, 2, 1), (4096, 100, 28)):
        assert lib.nvrx_work_words(R, K, S) == _native.work_words(R, K, S) == work_layout(R, K, S)["words"], (R, K, S)
        assert all(o % 4 == 0 for o in _native.work_offsets(R, K, S))
    fake = ctypes.c_void_p(4096)

    def groups(table=fake, R=8, K=8, S=2, tol=0.25, ppm=100000, out=fake):
        return lib.nvrx_work_groups(table, R, K, S, tol, ppm, out, None)

    assert groups(R=0) == _native.ERR_INVALID and b"shape" in lib.nvrx_last_error()
    assert groups(R=-1) == _native.ERR_INVALID and groups(K=-1) == _native.ERR_INVALID and groups(S=-1) == _native.ERR_INVALID
    assert groups(K=70000) == _native.ERR_RANGE and groups(S=70000) == _native.ERR_RANGE
    assert groups(R=4097) == _native.ERR_RANGE and b"at most 4096" in lib.nvrx_last_error()
    assert groups(R=4097, tol=-1.0) == _native.ERR_RANGE and b"at most 4096" in lib.nvrx_last_error()  # (the ranks first)
    assert groups(tol=-0.001) == _native.ERR_RANGE and b"count_tol" in lib.nvrx_last_error()
    assert groups(tol=16.001) == _native.ERR_RANGE and groups(tol=float("nan")) == _native.ERR_RANGE
    assert groups(ppm=-1) == _native.ERR_RANGE and b"max_unlike_ppm" in lib.nvrx_last_error()
    assert groups(ppm=1000001) == _native.ERR_RANGE
    assert groups(tol=99.0, ppm=-1) == _native.ERR_RANGE and b"count_tol" in lib.nvrx_last_error()
    assert groups(ppm=-1, table=None) == _native.ERR_RANGE  # (the parameters before the pointers)
    assert groups(table=None) == _native.ERR_INVALID and b"null" in lib.nvrx_last_error()
    assert groups(out=None) == _native.ERR_INVALID
    assert groups(out=ctypes.c_void_p(4100)) == _native.ERR_INVALID and b"aligned" in lib.nvrx_last_error()
    assert lib.nvrx_work_words(0, 1, 1) == _native.ERR_INVALID and lib.nvrx_work_words(4097, 1, 1) == _native.ERR_RANGE

    desc = _native.ReportDesc()
    desc.R, desc.K, desc.S = 8, 8, 2

    def report(ctx=fake, d=ctypes.byref(desc), tol=0.25, ppm=100000, out=fake):
        return lib.nvrx_report_work(ctx, d, tol, ppm, out)

    assert report(ctx=None) == _native.ERR_INVALID and report(d=None) == _native.ERR_INVALID
    assert report(tol=17.0) == _native.ERR_RANGE and report(ppm=2000000) == _native.ERR_RANGE
    assert report(out=None) == _native.ERR_INVALID and report(out=ctypes.c_void_p(4104)) == _native.ERR_INVALID


def test_the_args_check_program_runs_clean():
    """``make work-args-check``: both entries with invalid arguments only, host code under ASan + UBSan, a stand-alone program."""
    out = subprocess.run(["make", "-C", os.path.join(REPO, "nvidia-resiliency-ext_amd", "csrc"), "work-args-check"],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "work_args_check: 0 failure(s)" in out.stdout
