"""Slack scores, host side: the scenarios of the feature through ``ReportGenerator`` on the CPU checker backend, the rule,
the option's plumbing and errors, the columns, lifetime and pickling, the collectives of 2 and 3 gloo ranks, the Lightning
callback's switch and the stand-alone argument check.  No GPU."""
import ctypes
import importlib.util
import json
import os
import pickle
import subprocess

import numpy as np
import pytest

import mp_util
import slack_workers
from slack_oracle_backend import (ALLREDUCE, CALLS, COLS, NAN_BITS, RANKS, CountingSlackBackend, SlackOracleBackend,
                                  column_of, expected_scenario_records, named, play, slack_local_rows, slack_records)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RCCL_KEY = "_Z17rcclGenericKernelILi1ELb0EEv24ncclDevKernelArgsStorageILm4096EE"  # a device kernel of the installed librccl.so


@pytest.fixture
def cpu_backend():
    from nvrx_straggler import backend

    be = SlackOracleBackend()
    backend.set_backend(be)
    try:
        yield be
    finally:
        backend.set_backend(None)


def _as_dict(rec, ranks, keys, min_ranks=4, min_share=0.05, max_ratio=0.25):
    """What ``Report.slack_scores()`` must return for the records ``rec`` (written independently of the product's builder)."""
    job, cols, rk = rec
    tw, ts = (float(x) for x in job[:2].view(np.float32))
    out = {"ranks": {}, "typical_waited_us": tw, "typical_share": ts, "ranks_with_data": int(job[2]), "columns": {},
           "min_ranks": min_ranks, "min_share": min_share, "max_ratio": max_ratio}
    for i, r in enumerate(ranks):
        if rk[i, 5]:
            f = rk[i, :4].view(np.float32)
            out["ranks"][r] = {"collective_us": float(f[0]), "waited_us": float(f[1]), "compute_us": float(f[2]),
                               "share": float(f[3]), "calls": int(rk[i, 4]), "lead_us": tw - float(f[1])}
    for c in range(COLS):
        if cols[c, 0] != NAN_BITS:
            out["columns"][c] = {"floor_us": float(cols[c, :1].view(np.float32)[0]), "ranks": int(cols[c, 1]), "kernels": keys.get(c, [])}
    return out


def _blank_report(rank_to_node=None):
    from nvrx_straggler.reporting import Report

    return Report(gpu_relative_perf_scores={}, section_relative_perf_scores={}, gpu_individual_perf_scores={},
                  section_individual_perf_scores={}, local_section_summaries={}, local_kernel_summaries={},
                  generate_report_elapsed_time=0.0, gather_on_rank0=True, rank=0, rank_to_node=rank_to_node or {})


# ---- 1. the restatement on hand-made tables -----------------------------------------------------------------------------------
def test_the_restatement_on_a_table_worked_out_by_hand():
    slack = np.zeros((4, 2, COLS), dtype=np.float32)
    slack[:, 0, :] = -1.0
    # column 3: ranks 0..3 spend 100, 160, 160, 220 us per call over 10 calls; column 9: rank 0 alone
    slack[:, 0, 3], slack[:, 1, 3] = [1000.0, 1600.0, 1600.0, 2200.0], 10.0
    slack[0, 0, 9], slack[0, 1, 9] = 50.0, 5.0
    table = np.zeros((4, 2 * 2 + 1 + 1), dtype=np.float32)  # K = 1, S = 1
    table[:, 0], table[:, 4] = 7.0, [1000.0, 400.0, 400.0, 800.0]
    table[3, 0] = -1.0  # rank 3 has no statistics for kernel 0: its weight does not count
    job, cols, ranks = slack_records(slack, table, 1, 1, 4)
    f = ranks.view(np.float32)
    assert cols[3].tolist() == [np.float32(100.0).view(np.uint32), 4, 0, 0] and cols[9].tolist() == [NAN_BITS, 1, 0, 0]
    assert f[:, 0].tolist() == [1000.0, 1600.0, 1600.0, 2200.0] and f[:, 1].tolist() == [0.0, 600.0, 600.0, 1200.0]
    assert f[:, 2].tolist() == [1000.0, 400.0, 400.0, 0.0]
    assert f[:, 3].tolist() == [0.0, np.float32(600 / 2000), np.float32(600 / 2000), np.float32(1200 / 2200)]
    assert ranks[:, 4].tolist() == [10] * 4 and ranks[:, 5].tolist() == [1] * 4
    assert job[:2].view(np.float32).tolist() == [600.0, np.float32(0.3)] and job[2:].tolist() == [4, 1, 0, 0, 0, 0]  # LOWER medians
    # min_ranks 1: rank 0's own column counts too, with nothing above its floor
    job, cols, ranks = slack_records(slack, table, 1, 1, 1)
    assert cols[9].tolist() == [np.float32(10.0).view(np.uint32), 1, 0, 0] and ranks[0, 4:6].tolist() == [15, 2]
    assert ranks.view(np.float32)[0, :2].tolist() == [1050.0, 0.0] and job[3] == 2
    # nobody has data
    job, cols, ranks = slack_records(np.where(np.arange(2)[None, :, None] == 0, -1.0, 0.0).astype(np.float32).repeat(3, 0)
                                     .reshape(3, 2, 1).repeat(COLS, 2), None, 0, 0, 4)
    assert job.tolist() == [NAN_BITS, NAN_BITS, 0, 0, 0, 0, 0, 0] and (ranks[:, :4] == NAN_BITS).all() and not ranks[:, 4:].any()
    # the local step: rows beyond rows_active and rows without samples are left out; two rows of one column add up in row order
    stats = np.zeros((2 * 8, 8), dtype=np.float32)
    for q in range(2):
        stats[q * 8 + 1, 5:7] = 4, 40.0 + q
        stats[q * 8 + 2, 5:7] = 0, 0.0
        stats[q * 8 + 3, 5:7] = 2, 0.5
        stats[q * 8 + 6, 5:7] = 9, 99.0
    rows = slack_local_rows(stats, [1, 2, 3, 6], [63, 0, 63, 5], 6, 8, 2)
    assert rows[:, 0, 63].tolist() == [40.5, 41.5] and rows[:, 1, 63].tolist() == [6.0, 6.0]
    assert rows[:, :, 0].tolist() == [[-1.0, 0.0]] * 2 and rows[:, :, 5].tolist() == [[-1.0, 0.0]] * 2
    assert slack_local_rows(stats, [1, 2, 3, 6], [63, 0, 63, 5], 0, 8, 2)[:, :, 5].tolist() == [[99.0, 9.0]] * 2


# ---- 2. the scenarios ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("emulate_fused,asynchronous", [(False, False), (True, False), (True, True)])
def test_a_late_rank_is_named_and_nobody_else_is(emulate_fused, asynchronous):
    from nvrx_straggler import backend

    be = SlackOracleBackend(emulate_fused=emulate_fused)
    backend.set_backend(be)
    try:
        col = column_of(ALLREDUCE)
        for late, want in ((5, [5]), (None, [])):
            stats = []
            planned = []
            reports = play(be, late_rank=late, reports=2, stats_out=stats, asynchronous=asynchronous, planned_out=planned,
                           name_collectives=late is None)
            # the general path, then -- scenario 1 -- the cached plan (an asynchronous generator also runs its old plan when
            # the caller's table names a kernel without an id, which a collective kernel is)
            assert planned == [False, emulate_fused and (late is not None or asynchronous)]
            for rep, st in zip(reports, stats):
                s = rep.slack_scores()
                expected = expected_scenario_records(st)
                assert json.dumps(s, sort_keys=True) == json.dumps(_as_dict(expected, range(RANKS), {col: [ALLREDUCE]}), sort_keys=True)
                assert named(rep.identify_slack_stragglers()) == want
                assert named(rep.identify_stragglers()) == []
                assert min(rep.gpu_relative_perf_scores.values()) >= 0.99
                assert all(v >= 0.99 for sec in rep.section_relative_perf_scores.values() for v in sec.values())
                assert s["ranks_with_data"] == RANKS and list(s["columns"]) == [col] and s["columns"][col]["ranks"] == RANKS
                per_call = {r: rec["waited_us"] / CALLS for r, rec in s["ranks"].items()}
                assert all(rec["calls"] == CALLS and rec["compute_us"] == 1000.0 * CALLS for rec in s["ranks"].values())
                if late is None:
                    assert max(per_call.values()) <= 2.0 and max(rec["share"] for rec in s["ranks"].values()) <= 0.002
                else:
                    assert per_call[5] == 0.0 and s["ranks"][5]["lead_us"] == s["typical_waited_us"]
                    assert all(297.5 <= v <= 300.5 for r, v in per_call.items() if r != 5), per_call
                    assert all(0.1985 <= rec["share"] <= 0.2005 for r, rec in s["ranks"].items() if r != 5)
                    assert round(s["typical_share"], 3) == 0.199
        assert be.slack_local_calls == be.slack_score_calls == 4
        assert be.slack_args[-1] == (RANKS, 1, 1, 0, RANKS, 4) and be.slack_lists[-1] == ((2,), (col,))
    finally:
        backend.set_backend(None)


def test_the_rule_at_its_boundaries():
    def report(waited, share, **rule):
        r = _blank_report(rank_to_node={i: "n" for i in range(len(waited))})
        tw, ts = sorted(waited)[(len(waited) - 1) >> 1], sorted(share)[(len(share) - 1) >> 1]
        r.__dict__["_slack"] = {"ranks": {i: {"collective_us": 1.0, "waited_us": w, "compute_us": 0.0, "share": s, "calls": 1,
                                             "lead_us": tw - w} for i, (w, s) in enumerate(zip(waited, share))},
                                "typical_waited_us": tw, "typical_share": ts, "ranks_with_data": len(waited), "columns": {},
                                "min_ranks": 4, "min_share": rule.get("min_share", 0.05), "max_ratio": rule.get("max_ratio", 0.25)}
        return r

    r = report([100.0, 25.0, 100.0, 26.0, 100.0], [0.05, 0.0, 0.05, 0.01, 0.05])
    assert named(r.identify_slack_stragglers()) == [1]                       # 25 <= 0.25 * 100, 26 is not; share 0.05 >= 0.05
    assert named(r.identify_slack_stragglers(max_ratio=0.26)) == [1, 3]
    assert named(r.identify_slack_stragglers(min_share=0.0501)) == []
    assert named(r.identify_slack_stragglers(max_ratio=0)) == []
    assert named(report([0.0, 0.0, 0.0, 50.0], [0.0, 0.0, 0.0, 0.2]).identify_slack_stragglers(min_share=0)) == []  # typical wait 0
    assert named(report([100.0, 0.0, 100.0, 0.0], [0.2, 0.0, 0.2, 0.0]).identify_slack_stragglers()) == []       # half are late
    assert named(report([100.0, 0.0, 100.0, 0.0, 100.0], [0.2, 0.0, 0.2, 0.0, 0.2]).identify_slack_stragglers()) == [1, 3]
    assert named(report([100.0, 25.0, 100.0], [0.04, 0.0, 0.04]).identify_slack_stragglers()) == []  # the job does not wait enough
    got = r.identify_slack_stragglers()
    assert list(got) == ["straggler_gpus_slack"] and {(s.rank, s.node) for s in got["straggler_gpus_slack"]} == {(1, "n")}
    for bad in (-0.1, "x", True, float("nan")):
        with pytest.raises(ValueError, match="min_share must be a number >= 0"):
            r.identify_slack_stragglers(min_share=bad)
        with pytest.raises(ValueError, match="max_ratio must be a number >= 0"):
            r.identify_slack_stragglers(max_ratio=bad)
    assert _blank_report().slack_scores() == {} and _blank_report().identify_slack_stragglers() == {"straggler_gpus_slack": set()}


def test_the_smaller_delays_of_the_sketch(cpu_backend):
    for late_us, typical, want in ((100.0, 0.076, [5]), (60.0, 0.048, [])):
        # (the sketch drew these two with other seeds; the shares depend on the delay, not on the draw)
        rep = play(cpu_backend, late_rank=5, late_us=late_us)[0]
        s = rep.slack_scores()
        assert abs(s["typical_share"] - typical) <= 0.002, s["typical_share"]
        assert s["ranks"][5]["waited_us"] == 0.0 and named(rep.identify_slack_stragglers()) == want
        assert named(rep.identify_stragglers()) == []


# ---- 3. columns ---------------------------------------------------------------------------------------------------------------
def test_the_column_of_a_key_is_its_digest_modulo_64():
    from nvrx_straggler import _native, reporting
    from nvrx_straggler.name_mapper import name_digest

    assert reporting.SLACK_COLS == _native.SLACK_COLS == COLS == 64
    key = RCCL_KEY + "_blk_256_1_1_grid_64_1_1"
    pinned = {ALLREDUCE: 60, "ncclDevKernel_new": 43, key: 58}
    for k, col in pinned.items():
        assert reporting.slack_column(k) == col == name_digest(k) % 64 and reporting.is_collective_kernel(k)
    path = os.path.join(os.path.dirname(importlib.util.find_spec("torch").origin), "lib", "librccl.so")
    if os.path.exists(path):  # the pinned key is a kernel the installed library launches
        with open(path, "rb") as f:
            assert RCCL_KEY.encode() in f.read()
    rows, cols, keys = reporting.slack_row_list({"gemm": 0, ALLREDUCE: 7, "ncclDevKernel_new": 3, key: 5, "hipevent::x": 1,
                                                 "ncclDevKernel_z": 9, "ncclDevKernel_AllGather_RING_LL_x": 11})
    assert rows == [3, 5, 7, 9, 11] and cols[:4] == [43, 58, 60, 59]
    assert keys[43] == ("ncclDevKernel_new",) and sum(len(v) for v in keys.values()) == 5
    assert reporting.slack_row_list({"gemm": 0}) == ([], [], {})
    # keys that collide share a column, in row order
    pool = [f"ncclDevKernel_{i}" for i in range(200)]
    a = pool[0]
    b = next(k for k in pool[1:] if reporting.slack_column(k) == reporting.slack_column(a))
    rows, cols, keys = reporting.slack_row_list({b: 1, a: 4})
    assert rows == [1, 4] and cols[0] == cols[1] and keys[cols[0]] == (b, a)


# ---- 4. the option ------------------------------------------------------------------------------------------------------------
def test_option_values(cpu_backend, monkeypatch):
    from nvrx_straggler import Detector
    from nvrx_straggler.folded import FoldedJob
    from nvrx_straggler.reporting import ReportGenerator

    with pytest.raises(ValueError, match="collective_slack needs relative_perf_scores"):
        ReportGenerator(["individual_perf_scores"], collective_slack=True)
    for bad in (0, -1, 4.0, "4", None, True):
        with pytest.raises(ValueError, match="slack_min_ranks must be an integer >= 1"):
            ReportGenerator(["relative_perf_scores"], collective_slack=True, slack_min_ranks=bad)
    for bad in (-0.1, float("nan"), float("inf"), "x", None, True):
        with pytest.raises(ValueError, match="slack_min_share must be a finite number >= 0"):
            ReportGenerator(["relative_perf_scores"], collective_slack=True, slack_min_share=bad)
        with pytest.raises(ValueError, match="slack_max_ratio must be a finite number >= 0"):
            ReportGenerator(["relative_perf_scores"], collective_slack=True, slack_max_ratio=bad)
    gen = ReportGenerator(["relative_perf_scores"], collective_slack=True)
    assert (gen.collective_slack, gen.slack_min_ranks, gen.slack_min_share, gen.slack_max_ratio) == (True, 4, 0.05, 0.25)
    gen = ReportGenerator(["relative_perf_scores"], collective_slack=1, slack_min_ranks=2, slack_min_share=0, slack_max_ratio=1)
    assert (gen.collective_slack, gen.slack_min_ranks, gen.slack_min_share, gen.slack_max_ratio) == (True, 2, 0.0, 1.0)
    off = ReportGenerator(["individual_perf_scores"], slack_min_ranks=-5, slack_min_share="x")  # (ignored while off)
    assert off.collective_slack is False
    assert len(__import__("nvrx_straggler").row_families.FAMILIES) == 4  # a sibling step, not a row family
    # the environment variable is the Detector's default, read only when the argument is None
    monkeypatch.setenv("NVRX_COLLECTIVE_SLACK", "1")
    Detector.initialize(node_name="n0")
    try:
        r = Detector.reporter
        assert (r.collective_slack, r.slack_min_ranks, r.slack_min_share, r.slack_max_ratio) == (True, 4, 0.05, 0.25)
    finally:
        Detector.shutdown()
    Detector.initialize(node_name="n0", collective_slack=False)
    try:
        assert Detector.reporter.collective_slack is False
    finally:
        Detector.shutdown()
    monkeypatch.setenv("NVRX_COLLECTIVE_SLACK", "0")
    Detector.initialize(node_name="n0")
    try:
        assert Detector.reporter.collective_slack is False
    finally:
        Detector.shutdown()
    monkeypatch.delenv("NVRX_COLLECTIVE_SLACK")
    Detector.initialize(node_name="n0", collective_slack=True, slack_min_ranks=2, slack_min_share=0.1, slack_max_ratio=0.5)
    try:
        r = Detector.reporter
        assert (r.collective_slack, r.slack_min_ranks, r.slack_min_share, r.slack_max_ratio) == (True, 2, 0.1, 0.5)
    finally:
        Detector.shutdown()
    Detector.initialize(node_name="n0")
    try:
        assert Detector.reporter.collective_slack is False
    finally:
        Detector.shutdown()
    job = FoldedJob(total_ranks=2, sections=1, ring_cap=16, scores_to_compute=("relative_perf_scores",), collective_slack=True,
                    slack_min_ranks=2, kernel_names=["k", ALLREDUCE])
    try:
        assert job.reporter.collective_slack and job.reporter.slack_min_ranks == 2 and job.rings.rows_per_rank == 3
        for lr in range(2):
            job.rings.push_many(0, [5.0, 5.0], lr=lr)
            job.load_kernels(lr, [[1.0, 1.0], [10.0 + 5 * lr] * 2])
        s = job.report().slack_scores()
        assert s["ranks"][0]["waited_us"] == 0.0 and s["ranks"][1]["waited_us"] == 10.0 and s["min_ranks"] == 2
    finally:
        job.close()


def test_option_needs_a_backend_with_slack_scores():
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator
    from trend_oracle_backend import TrendOracleBackend

    be = TrendOracleBackend()
    backend.set_backend(be)
    try:
        with pytest.raises(RuntimeError, match="no slack scores"):
            ReportGenerator(["relative_perf_scores"], collective_slack=True)
        ReportGenerator(["relative_perf_scores"])
    finally:
        backend.set_backend(None)


@pytest.mark.parametrize("emulate_fused,asynchronous", [(False, False), (True, False), (True, True)])
def test_default_is_off_and_calls_nothing(emulate_fused, asynchronous):
    from nvrx_straggler import Statistic as S
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator

    be = CountingSlackBackend(emulate_fused=emulate_fused)
    backend.set_backend(be)
    try:
        gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=True, node_name="n",
                              asynchronous=asynchronous)
        summ = {S.MIN: 1.0, S.MAX: 2.0, S.MED: 1.5, S.AVG: 1.5, S.STD: 0.1, S.NUM: 4}
        rep = gen.generate_report({"sec": summ}, {"k": summ, ALLREDUCE: summ})
        assert rep.slack_scores() == {} and pickle.loads(pickle.dumps(rep)).slack_scores() == {}
        assert rep.identify_slack_stragglers() == {"straggler_gpus_slack": set()}
        rings = be.make_rings(1, 8, 16)
        rows = {"sec": rings.row_for(0, "sec")}
        krows = {"k": rings.row_for(1, "k"), ALLREDUCE: rings.row_for(1, ALLREDUCE)}
        for i in range(3):
            for row in (0, 1, 2):
                rings.push_many(row, [5.0 + i, 6.0])
            rep = gen.generate_report_from_rings(rings, rows, krows)
            rings.reset()
            assert rep.slack_scores() == {} and "_slack" not in rep.__dict__
        assert gen._ring_plan is not None and be.slack_calls == 0
        gen.close()
        # ... and the dict-input report carries none with the option on either
        on = ReportGenerator(["relative_perf_scores"], gather_on_rank0=True, node_name="n", collective_slack=True)
        assert on.generate_report({"sec": summ}, {"k": summ, ALLREDUCE: summ}).slack_scores() == {} and be.slack_calls == 0
        on.close()
    finally:
        backend.set_backend(None)


# ---- 5. lifetime and pickling -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("emulate_fused,asynchronous", [(False, False), (True, False), (True, True)])
def test_a_held_report_keeps_its_slack_scores_and_reports_travel(emulate_fused, asynchronous):
    from nvrx_straggler import backend

    be = SlackOracleBackend(emulate_fused=emulate_fused)
    backend.set_backend(be)
    try:
        from nvrx_straggler.reporting import ReportGenerator

        gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=True, node_name="n", collective_slack=True,
                              slack_min_ranks=1, asynchronous=asynchronous)
        rings = be.make_rings(2, 4, 16)
        rows = {"sec": rings.row_for(0, "sec")}
        krows = {"k": rings.row_for(1, "k"), ALLREDUCE: rings.row_for(1, ALLREDUCE)}
        held = []
        for i in range(3):
            for lr in range(2):
                rings.push_many(0, [5.0, 5.0], lr=lr)
                rings.push_many(1, [1.0, 1.0], lr=lr)
                rings.push_many(2, [10.0 * (i + 1) + 7.0 * lr] * 2, lr=lr)
            held.append(gen.generate_report_from_rings(rings, rows, krows, local_ranks=2))
            rings.reset()
        assert all(h.reads == 0 for h in be.slack_handles)  # unread: nothing was waited for
        first = held[0].slack_scores()  # read after the next two were issued: still its own
        assert first["ranks"][0]["collective_us"] == 20.0 and first["ranks"][1]["waited_us"] == 14.0
        assert held[2].slack_scores()["ranks"][0]["collective_us"] == 60.0
        assert [h.reads for h in be.slack_handles] == [1, 0, 1]
        first["ranks"].clear()  # a private copy each time
        assert held[0].slack_scores()["ranks"] and be.slack_handles[0].reads == 1
        travelled = pickle.loads(pickle.dumps(held[1]))  # materialised on the way
        assert be.slack_handles[1].reads == 1
        assert travelled.slack_scores() == held[1].slack_scores() and travelled.slack_scores()["ranks"][0]["collective_us"] == 40.0
        # (two ranks: the lower median of their waits is the smaller one, 0 -- nobody is named)
        assert named(travelled.identify_slack_stragglers()) == named(held[1].identify_slack_stragglers()) == []
        assert named(travelled.identify_slack_stragglers(min_share=0, max_ratio=0)) == []
        assert isinstance(travelled.__dict__["_slack"], dict)
        gen.close()
    finally:
        backend.set_backend(None)


# ---- 6. several ranks: the same collectives everywhere ------------------------------------------------------------------------
@pytest.mark.parametrize("world,gather,emulate_fused,asynchronous", [(2, True, False, False), (3, False, False, False),
                                                                     (3, True, True, False), (2, False, True, True)])
def test_every_rank_issues_the_same_collectives(world, gather, emulate_fused, asynchronous):
    res = mp_util.run_ranks(slack_workers.ring_reports_recorded, world, gather_on_rank0=gather, emulate_fused=emulate_fused,
                            asynchronous=asynchronous)
    off = mp_util.run_ranks(slack_workers.ring_reports_recorded, world, gather_on_rank0=gather, emulate_fused=emulate_fused,
                            asynchronous=asynchronous, slack=False)
    for r in range(1, world):
        assert res[r]["calls"] == res[0]["calls"], (r, res[r]["calls"], res[0]["calls"])
    for i in range(6):
        # one more row gather than with the option off, of this rank's 2 x 64 floats, in every report on every rank
        # (the first report with the option off also agrees on the exchange route: a flag that reports with slack never ask for)
        extra = [c for c in res[0]["calls"][i] if c == ("rows", 2 * COLS)]
        without = [c for c in off[0]["calls"][i] if c[0] != "flag"]
        assert len(extra) == 1 and res[0]["calls"][i] == without + [("rows", 2 * COLS)], (i, res[0]["calls"][i], off[0]["calls"][i])
        assert res[0]["calls"][i][-1] == ("rows", 2 * COLS)  # behind the report's own collectives
    col = column_of(ALLREDUCE)
    for r in range(world):
        assert res[r]["local_calls"] == 6 and off[r]["local_calls"] == off[r]["score_calls"] == 0
        assert res[r]["score_calls"] == (6 if (not gather or r == 0) else 0)  # the rank without a report gathers and stops
        assert "collective_slack is set: reports with slack scores do not use the in-stream routes" in res[r]["route"]
        for i, entry in enumerate(res[r]["reports"]):
            if gather and r != 0:
                assert entry["slack"] is None
                continue
            s = entry["slack"]
            assert entry["pickled_same"] and s["ranks_with_data"] == world and s["min_ranks"] == min(4, world)
            assert sorted(s["ranks"]) == (list(range(world)) if gather else [r])
            assert s["columns"][col]["ranks"] == world and s["columns"][col]["kernels"] == [ALLREDUCE]
            # rank 0 spends 200 us per call in the all-reduce, rank q 200 + 100 q: the others wait for rank 0
            # (two ranks: the lower median of their waits is rank 0's own, 0, and nobody is named)
            assert entry["named"] == ([0] if world > 2 and (gather or r == 0) else [])
            if i >= 4:  # rank 0's new collective kernel: one rank has it, so its column is not referenced
                new = column_of("ncclDevKernel_new")
                assert new not in s["columns"] and (r != 0 or res[r]["lists"][i][1] == (col, new))
    with_tail = mp_util.run_ranks(slack_workers.ring_reports_recorded, 2, gather_on_rank0=True, tail=0.95)
    assert "tail_quantile is set" in with_tail[0]["route"]  # a row family that is also on keeps being named first
    assert with_tail[0]["calls"] == with_tail[1]["calls"] and with_tail[0]["calls"][0][-1] == ("rows", 2 * COLS)


# ---- 7. the Lightning callback ------------------------------------------------------------------------------------------------
def test_callback_warns_of_a_rank_the_others_wait_for_and_never_halts_for_it(monkeypatch):
    import callback_script
    import nvrx_straggler
    from nvidia_resiliency_ext.ptl_resiliency import StragglerDetectionCallback
    from nvrx_straggler.reporting import Report

    healthy = callback_script._scores(8)
    base = {k: v for k, v in callback_script.reports(8)[1].items() if not k.startswith("gpu_")}
    sequence = [None, {5: 0.0}, None, {}, {5: 10.0, 2: 0.0}, "weak"]

    def slack_of(e):
        if e == "weak":  # the job hardly waits: nobody is named
            waited, share = {r: 10.0 for r in range(8)}, 0.001
            waited[3] = 0.0
        else:
            waited, share = {r: 60000.0 for r in range(8)}, 0.2
            waited.update(e)
        return {"ranks": {r: {"collective_us": 100000.0, "waited_us": w, "compute_us": 200000.0, "share": w / 300000.0, "calls": 200,
                              "lead_us": sorted(waited.values())[3] - w} for r, w in waited.items()},
                "typical_waited_us": sorted(waited.values())[3], "typical_share": share, "ranks_with_data": 8, "columns": {},
                "min_ranks": 4, "min_share": 0.05, "max_ratio": 0.25}

    def scripted(n_ranks):
        return [None if e is None else dict(base, gpu_relative_perf_scores=healthy, gpu_individual_perf_scores=healthy,
                                            slack=slack_of(e)) for e in sequence]

    def make_report(slack=None, **fields):
        rep = Report(**fields)
        rep.__dict__["_slack"] = slack
        return rep

    monkeypatch.setattr(callback_script, "reports", scripted)
    monkeypatch.setitem(callback_script.CONFIGS, "waited", dict(callback_script.CONFIGS["print2_log_stop"], warn_if_waited_for=True))
    got = callback_script.drive(StragglerDetectionCallback, nvrx_straggler, make_report,
                                ("waited", "waited", 8, 0, False, False, False))
    assert got["initialize_calls"] == [dict(scores_to_compute=["relative_perf_scores", "individual_perf_scores"],
                                            gather_on_rank0=True, profiling_interval=1, report_time_interval=1.0,
                                            collective_slack=True)]
    its = got["iterations"]
    warnings = [[m for level, m in it["records"] if level == "WARNING"] for it in its]
    assert [len(w) for w in warnings] == [0, 1, 0, 0, 1, 0]  # one warning per report that names anybody
    assert warnings[1] == ["STRAGGLER DETECTION WARNING: The job waits for some GPUs in its collectives (slow host?): rank 5 (the "
                           "others wait 60000 us per window for it); the typical rank spends 20.0 % of its traced GPU time waiting"]
    assert "rank 2 (the others wait 60000 us" in warnings[4][0] and "rank 5 (the others wait 59990 us" in warnings[4][0]
    assert [it["should_stop"] for it in its] == [False] * len(sequence) and all(it["exit"] is None for it in its)  # stop_if_detected=True

    # the default, given or not: the initialize call and the transcript of today
    monkeypatch.undo()
    monkeypatch.setitem(callback_script.CONFIGS, "explicit_off", dict(callback_script.CONFIGS["print2_log_stop"], warn_if_waited_for=False))
    plain = callback_script.drive(StragglerDetectionCallback, nvrx_straggler, Report, callback_script.SCENARIOS[0])
    given = callback_script.drive(StragglerDetectionCallback, nvrx_straggler, Report,
                                  ("rank0_8ranks", "explicit_off", 8, 0, False, False, False))
    assert json.dumps(dict(given, config=None), sort_keys=True) == json.dumps(dict(plain, config=None), sort_keys=True)
    assert given["initialize_calls"] == [dict(scores_to_compute=["relative_perf_scores", "individual_perf_scores"],
                                              gather_on_rank0=True, profiling_interval=1, report_time_interval=1.0)]
    with pytest.raises(ValueError, match="warn_if_waited_for needs calc_relative_gpu_perf"):
        StragglerDetectionCallback(**dict(callback_script.CONFIGS["print3_indiv_only_log"], warn_if_waited_for=True))


# ---- 8. header, bindings and macros agree; the C entry points check their arguments before any device is touched ----------------
def test_entry_points_check_their_arguments_without_a_device():
    import re

    from nvrx_straggler import _native

    lib = _native.load()
    assert {"nvrx_slack_score", "nvrx_slack_local"} <= {name for name, _, _ in _native.SYMBOLS}
    assert lib.nvrx_abi_version() == 2
    header = open(os.path.join(REPO, "include", "nvrx_straggler.h")).read()
    assert re.search(r"#define NVRX_ABI_VERSION 2\b", header) and re.search(r"#define NVRX_SLACK_COLS 64\b", header)
    assert "#define NVRX_SLACK_WORDS(R) (8 + 4 * (size_t)NVRX_SLACK_COLS + 8 * (size_t)(R))" in header
    assert _native.slack_words(8) == 8 + 256 + 64 and _native.SLACK_HEAD_WORDS == 264 and _native.SLACK_RANK_WORDS == 8
    flat = " ".join(header.split())
    assert ("int nvrx_slack_score(const float *d_slack, const float *d_table, int R, int K, int S, int min_ranks, void *d_out, "
            "void *stream);") in flat
    assert ("int nvrx_slack_local(nvrx_ctx *ctx, const nvrx_report_desc *desc, const float *d_stats, const int32_t *rows, "
            "const int32_t *cols, int n, float *d_send, int rows_active, void *stream);") in flat
    fake = ctypes.c_void_p(4096)

    def score(slack=fake, table=fake, R=8, K=5, S=2, min_ranks=4, out=fake):
        return lib.nvrx_slack_score(slack, table, R, K, S, min_ranks, out, None)

    assert score(R=0) == _native.ERR_INVALID and score(K=-1) == _native.ERR_INVALID and score(S=-1) == _native.ERR_INVALID
    assert b"shape" in lib.nvrx_last_error()
    assert score(R=65537) == _native.ERR_RANGE and score(K=65537) == _native.ERR_RANGE and score(S=65537) == _native.ERR_RANGE
    assert score(min_ranks=0) == _native.ERR_RANGE and b"min_ranks" in lib.nvrx_last_error()
    assert score(slack=None) == _native.ERR_INVALID and score(table=None) == _native.ERR_INVALID and score(out=None) == _native.ERR_INVALID
    assert b"null" in lib.nvrx_last_error()
    assert score(slack=ctypes.c_void_p(4100)) == _native.ERR_INVALID and b"aligned" in lib.nvrx_last_error()
    assert score(out=ctypes.c_void_p(4104)) == _native.ERR_INVALID

    rows, cols = (ctypes.c_int32 * 3)(1, 2, 5), (ctypes.c_int32 * 3)(0, 63, 7)

    def local(ctx=fake, stats=fake, rows=rows, cols=cols, n=3, send=fake):
        return lib.nvrx_slack_local(ctx, None, stats, rows, cols, n, send, 0, None)

    assert local(ctx=None) == _native.ERR_INVALID and local(send=None) == _native.ERR_INVALID and local(n=-1) == _native.ERR_INVALID
    assert local(rows=None) == _native.ERR_INVALID and local(cols=None) == _native.ERR_INVALID
    assert local(rows=(ctypes.c_int32 * 3)(-1, 2, 5)) == _native.ERR_RANGE and b"rows[0]" in lib.nvrx_last_error()
    assert local(cols=(ctypes.c_int32 * 3)(0, 64, 7)) == _native.ERR_RANGE and b"cols[1]" in lib.nvrx_last_error()
    assert local(rows=(ctypes.c_int32 * 3)(1, 5, 2)) == _native.ERR_INVALID and b"ascending" in lib.nvrx_last_error()
    assert local(stats=None) == _native.ERR_INVALID and local(send=ctypes.c_void_p(4100)) == _native.ERR_INVALID


def test_the_stand_alone_argument_check_passes_under_the_sanitizers():
    """``make slack-args-check``: both entry points with invalid arguments only, host code under ASan + UBSan."""
    res = subprocess.run(["make", "-C", os.path.join(REPO, "nvidia-resiliency-ext_amd", "csrc"), "slack-args-check"],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "slack_args_check: 0 failure(s)" in res.stdout
