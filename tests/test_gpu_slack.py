"""GPU parity of the slack-score kernels (``k_slack_local``, ``k_slack_cols``, ``k_slack_rank``, ``k_slack_job`` in its three
forms) through the C ABI and the backend, and of the slack step of a report, against the restatement of
tests/slack_oracle_backend.py.  Every record of every case is compared.

Bounds: send rows of the local step and column records bit for bit (one fixed sequence of f64 additions; a minimum and a
count); NaN and inf masks equal; counts exact; the floats of rank and job records within 2e-6 * max(1, |expected|), the bound
tests/test_gpu_robust.py and tests/test_gpu_tail.py use for f64 sums taken in another order (64 terms here, each exact or
one rounding away: 64 * 2^-53 relative, far inside); the case with power-of-two counts and integer weights below 2^24 has
exact quotients and sums and is compared bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import slack_workers
from mp_util import run_ranks
from score_cases import random_table
from slack_oracle_backend import (ALLREDUCE, CALLS, COLS, NAN_BITS, RANKS, column_of, expected_scenario_records, named, play,
                                  slack_local_rows, slack_records)

pytestmark = pytest.mark.gpu

RANK_COUNTS = (1, 2, 3, 4, 63, 64, 65, 100, 1025)


@pytest.fixture(scope="module")
def be():
    from nvrx_straggler.backend import get_backend

    return get_backend()


# ---- 1. k_slack_local ---------------------------------------------------------------------------------------------------------
ROWS_PER_RANK, ROWS_ACTIVE = 272, 262


def _lists():
    """(row, column) lists of 0, 1, 2, 65 and 257 collective rows: columns 0 and 63, two rows in one column, a row at
    rows_active and one beyond (ignored), rows without samples (row % 4 == 0 holds none)."""
    rng = np.random.default_rng(11)
    out = {0: ([], []), 1: ([5], [63]), 2: ([3, 9], [17, 17]), "2b": ([4, 261], [0, 63])}  # (row 4 holds no sample)
    for n in (65, 257):
        rows = sorted(rng.permutation(ROWS_ACTIVE)[: n - 2].tolist() + [ROWS_ACTIVE, 270])
        cols = rng.integers(0, COLS, n).tolist()
        cols[0], cols[1] = 0, 63
        out[n] = (rows, cols)
    return out


@pytest.mark.parametrize("local_ranks", [1, 3])
def test_local_step_matches_the_restatement_bit_for_bit(be, local_ranks):
    from nvrx_straggler import _native

    lib = be.lib
    rings = be.make_rings(local_ranks, ROWS_PER_RANK, 16)
    try:
        for r in range(ROWS_PER_RANK):
            rings.alloc_row(1)
        rng = np.random.default_rng(local_ranks)
        rows, values = [], []
        for q in range(local_ranks):
            for r in range(ROWS_PER_RANK):
                n = (r % 4) * 3  # 0, 3, 6 or 9 samples
                rows += [q * ROWS_PER_RANK + r] * n
                values += rng.lognormal(5.0, 0.3, n).astype(np.float32).tolist()
        rings.push_pairs(np.array(rows), np.array(values))
        ws = be.workspace(local_ranks, 1, 1, local_ranks, local_ranks * ROWS_PER_RANK)
        rings.report_local(ws, True, rows_active=ROWS_ACTIVE)
        be.synchronize()
        stats = ws.stats_dev.cpu().numpy().copy()  # the rows the kernel reads, read back from the device
        assert (stats[: ROWS_ACTIVE, 5] == np.tile([0, 3, 6, 9], ROWS_PER_RANK // 4 + 1)[:ROWS_ACTIVE]).all()  # NUM is written, 0 for an empty row
        send = torch.full((local_ranks, 2 * COLS), 7.0, dtype=torch.float32, device=be.device)

        def local(rows, cols, rows_active=ROWS_ACTIVE, d_stats=ws.d_stats, desc=None):
            r, c = np.asarray(rows, dtype=np.int32), np.asarray(cols, dtype=np.int32)
            return lib.nvrx_slack_local(rings.ctx, desc, d_stats, r.ctypes.data, c.ctypes.data, r.size, send.data_ptr(),
                                        rows_active, be._stream_handle)

        for tag, (rows, cols) in list(_lists().items()) + [("again", _lists()[257])]:  # (the last: the list is not uploaded again)
            send.fill_(7.0)
            torch.cuda.synchronize()
            assert local(rows, cols) == 0, lib.nvrx_last_error()
            be.synchronize()
            got = send.cpu().numpy().reshape(local_ranks, 2, COLS)
            exp = slack_local_rows(stats, rows, cols, ROWS_ACTIVE, ROWS_PER_RANK, local_ranks)
            assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), (tag, np.argwhere(got.view(np.uint32) != exp.view(np.uint32))[:8])
            if tag == 257:
                assert (exp[:, 1] > 0).sum() > 40 * local_ranks and (exp[:, 1].max(axis=1) > 9).all()  # rows did add up in a column
        assert ws.stats_dev.cpu().numpy().tobytes() == stats.tobytes()  # it reads the statistics, and only reads them
        # what depends on the context's geometry (the stand-alone program covers the rest): nothing of it reaches the device
        assert local(list(range(ROWS_PER_RANK)) + [ROWS_PER_RANK], [0] * (ROWS_PER_RANK + 1)) == _native.ERR_INVALID
        assert local([1, ROWS_PER_RANK], [0, 0]) == _native.ERR_RANGE and b"rows[1]" in lib.nvrx_last_error()
        assert local([1], [0], rows_active=-1) == _native.ERR_INVALID and local([1], [0], rows_active=ROWS_PER_RANK + 1) == _native.ERR_INVALID
        assert local([1], [0], desc=ws.block.desc_ref, d_stats=None) == _native.ERR_STATE and b"descriptor" in lib.nvrx_last_error()
    finally:
        rings.close()


# ---- 2. nvrx_slack_score -------------------------------------------------------------------------------------------------------
def _slack_table(rng, R, sparse):
    """Gathered rows [R, 2, 64] with the special columns: 0 and 63 present everywhere, 1 on one rank, 2 nowhere, 3 equal
    everywhere (ties at the median), 4 with a zero and a +inf among ordinary values, 5 with NaN times; the rest present on
    70 % of the ranks -- or, ``sparse``, only columns 10..20 on half the ranks, so that columns go unreferenced and ranks are
    left without data."""
    t = np.full((R, COLS), -1.0, dtype=np.float32)
    n = np.zeros((R, COLS), dtype=np.float32)
    calls = rng.integers(1, 300, (R, COLS)).astype(np.float32)
    per_call = rng.lognormal(5.3, 0.4, (R, COLS))
    if sparse:
        on = np.zeros((R, COLS), dtype=bool)
        on[:, 10:21] = rng.random((R, 11)) < 0.5
    else:
        on = rng.random((R, COLS)) < 0.7
        on[:, [0, 3, 4, 5, 63]] = True
        on[:, [1, 2]] = False
        on[rng.integers(R), 1] = True
    t[on], n[on] = (calls * per_call).astype(np.float32)[on], calls[on]
    if not sparse:
        t[:, 3], n[:, 3] = 4096.0, 32.0
        t[0, 4] = 0.0
        t[R - 1, 4] = np.inf if R > 1 else 0.0
        t[rng.random(R) < 0.3, 5] = np.nan
        t[R // 2, 5] = np.nan
    return np.stack([t, n], axis=1)


def _exact_table(rng, R):
    """Power-of-two counts and integer per-call times: every quotient, product and sum is exact."""
    n = (2.0 ** rng.integers(0, 9, (R, COLS))).astype(np.float32)
    avg = rng.integers(1, 512, (R, COLS)).astype(np.float32)
    t = n * avg  # < 2^17 each: 64 of them stay below 2^24
    off = rng.random((R, COLS)) < 0.25
    t[off], n[off] = -1.0, 0.0
    return np.stack([t, n], axis=1)


def _score(be, slack, T, K, S, min_ranks, first_rank=0, n_ranks=None):
    R = slack.shape[0]
    ws = be.workspace(R, K, S, R, 0)
    ws.slack_settle()
    ws.send.copy_(torch.from_numpy(T))
    send, table, _ = ws.slack_buffers()
    assert send is table
    table.copy_(torch.from_numpy(slack.reshape(R, 2 * COLS)))
    torch.cuda.synchronize()
    return be.slack_score(ws, table, ws.send, first_rank, n_ranks, min_ranks).records()


def _compare(got, exp, tag, exact=False):
    (gj, gc, gr), (ej, ec, er) = got, exp
    assert gj.shape == ej.shape and gc.shape == ec.shape and gr.shape == er.shape, tag
    assert np.array_equal(gc, ec), (tag, "columns", np.argwhere(gc != ec)[:8].tolist())
    assert np.array_equal(gr[:, 4:], er[:, 4:]) and np.array_equal(gj[2:], ej[2:]), (tag, "counts", gj, ej)
    if exact:
        assert np.array_equal(gr, er) and np.array_equal(gj, ej), (tag, "exact", np.argwhere(gr != er)[:8].tolist(), gj, ej)
        return 0.0
    worst = 0.0
    for what, g, e in (("ranks", gr[:, :4], er[:, :4]), ("job", gj[:2], ej[:2])):
        g, e = np.ascontiguousarray(g).view(np.float32).astype(np.float64), np.ascontiguousarray(e).view(np.float32).astype(np.float64)
        assert np.array_equal(np.isnan(g), np.isnan(e)), (tag, what, "NaN masks", np.argwhere(np.isnan(g) != np.isnan(e))[:8].tolist())
        assert np.array_equal(np.isposinf(g), np.isposinf(e)) and np.array_equal(np.isneginf(g), np.isneginf(e)), (tag, what, "inf masks")
        fin = np.isfinite(e)
        if fin.any():
            err = float((np.abs(g[fin] - e[fin]) / np.maximum(1.0, np.abs(e[fin]))).max())
            worst = max(worst, err)
            assert err <= 2e-6, (tag, what, err)
    return worst


@pytest.mark.parametrize("R", RANK_COUNTS)
def test_score_step_matches_the_restatement(be, R):
    S = 2
    worst = 0.0
    for K in (0, 5):
        for sparse in (False, True):
            rng = np.random.default_rng(1000 * R + 10 * K + sparse)
            slack, T = _slack_table(rng, R, sparse), random_table(rng, R, K, S)
            for min_ranks in (1, 4):
                exp = slack_records(slack, T, K, S, min_ranks)
                tag = (R, K, min_ranks, "sparse" if sparse else "dense")
                worst = max(worst, _compare(_score(be, slack, T, K, S, min_ranks), exp, tag))
                if not sparse:
                    present = exp[1][:, 1]
                    assert present[0] == present[63] == present[3] == R and present[1] == 1 and present[2] == 0
                    assert present[5] < R or R == 1
                elif R >= 63 and min_ranks == 4:
                    assert 0 < exp[0][3] <= 11 and (exp[1][:10, 0] == NAN_BITS).all()
    print("R", R, "rank and job floats: max error", worst)


def test_score_step_on_ranks_without_data_and_a_slice_of_the_ranks(be):
    rng = np.random.default_rng(5)
    for R in (8, 100, 1025):
        slack = _slack_table(rng, R, True)
        slack[::3, 0, :], slack[::3, 1, :] = -1.0, 0.0  # every third rank holds nothing at all
        T = random_table(rng, R, 5, 2)
        exp = slack_records(slack, T, 5, 2, 4)
        assert 0 < exp[0][2] < R and (exp[2][::3, :4] == NAN_BITS).all() and not exp[2][::3, 4:].any()
        _compare(_score(be, slack, T, 5, 2, 4), exp, (R, "holes"))
        lo, n = R // 2, R - R // 2 - 1
        got = _score(be, slack, T, 5, 2, 4, lo, n)  # the head and the slice of the ranks a report covers
        _compare(got, (exp[0], exp[1], exp[2][lo : lo + n]), (R, "slice"))
    # nobody has a referenced column
    slack = _slack_table(rng, 8, True)
    slack[:, 0, :], slack[:, 1, :] = -1.0, 0.0
    slack[2, 0, 7], slack[2, 1, 7] = 10.0, 1.0
    got = _score(be, slack, random_table(rng, 8, 5, 2), 5, 2, 4)
    assert got[0].tolist() == [NAN_BITS, NAN_BITS, 0, 0, 0, 0, 0, 0] and (got[2][:, :4] == NAN_BITS).all() and got[1][7].tolist() == [NAN_BITS, 1, 0, 0]
    # K = 0 needs no table
    slack = _exact_table(rng, 8)
    ws = be.workspace(8, 0, 2, 8, 0)
    _, table, out = ws.slack_buffers()
    table.copy_(torch.from_numpy(slack.reshape(8, 2 * COLS)))
    torch.cuda.synchronize()
    assert be.lib.nvrx_slack_score(table.data_ptr(), None, 8, 0, 2, 4, out.data_ptr(), be._stream_handle) == 0
    be.synchronize()
    host = out.cpu().numpy().view(np.uint32)
    exp = slack_records(slack, None, 0, 2, 4)
    assert np.array_equal(host[:8], exp[0]) and np.array_equal(host[8:264].reshape(64, 4), exp[1])
    assert np.array_equal(host[264 : 264 + 64].reshape(8, 8), exp[2])


@pytest.mark.parametrize("R", [8, 64, 100, 1025])
def test_exact_inputs_give_exact_records(be, R):
    rng = np.random.default_rng(R)
    slack = _exact_table(rng, R)
    T = random_table(rng, R, 5, 2)
    T[:, 2 * 7 : 2 * 7 + 5] = rng.integers(0, 1 << 20, (R, 5)).astype(np.float32)  # integer weights: the compute sum is exact too
    for min_ranks in (1, 4):
        _compare(_score(be, slack, T, 5, 2, min_ranks), slack_records(slack, T, 5, 2, min_ranks), (R, min_ranks, "exact"), exact=True)


# ---- 3. the step of a report ----------------------------------------------------------------------------------------------------
def _close(a, b):
    return a == b or abs(a - b) <= 2e-6 * max(1.0, abs(b))


@pytest.mark.parametrize("name_collectives", [True, False])
@pytest.mark.parametrize("asynchronous", [False, True])
def test_the_step_names_the_late_rank_stepwise_and_one_call(be, asynchronous, name_collectives):
    col = column_of(ALLREDUCE)
    for late, want in ((5, [5]), (None, [])):
        stats, planned = [], []
        reports = play(be, late_rank=late, reports=3, stats_out=stats, asynchronous=asynchronous, name_collectives=name_collectives,
                       planned_out=planned)
        # the caller names the all-reduce (as the Detector does): every report is stepwise (an asynchronous generator also runs
        # its old plan when the table names a kernel without an id, which a collective kernel is); else report 0 is stepwise,
        # then comes the one-call report
        assert planned == ([False] * 3 if name_collectives and not asynchronous else [False, True, True])
        for i, (rep, st) in enumerate(zip(reports, stats)):
            s = rep.slack_scores()
            job, cols, ranks = expected_scenario_records(st)
            f = ranks[:, :4].view(np.float32)
            assert named(rep.identify_slack_stragglers()) == want and named(rep.identify_stragglers()) == [], (i, s)
            assert min(rep.gpu_relative_perf_scores.values()) >= 0.99
            assert sorted(s["ranks"]) == list(range(RANKS)) and s["ranks_with_data"] == RANKS == int(job[2])
            assert list(s["columns"]) == [col] and s["columns"][col] == {
                "floor_us": float(cols[col, :1].view(np.float32)[0]), "ranks": RANKS, "kernels": [ALLREDUCE]}
            for r in range(RANKS):
                rec = s["ranks"][r]
                assert rec["calls"] == CALLS == int(ranks[r, 4])
                for j, key in enumerate(("collective_us", "waited_us", "compute_us", "share")):
                    assert _close(rec[key], float(f[r, j])), (i, r, key, rec[key], float(f[r, j]))
            assert _close(s["typical_waited_us"], float(job[:1].view(np.float32)[0]))
            assert _close(s["typical_share"], float(job[1:2].view(np.float32)[0]))
            if late is not None:
                assert s["ranks"][5]["waited_us"] == 0.0 and round(s["typical_share"], 3) == 0.199


def test_statistics_and_table_are_the_same_bytes_with_the_option_on_and_off(be):
    from nvrx_straggler.reporting import ReportGenerator
    from slack_oracle_backend import GEMM, scenario

    step, gemm, coll = scenario(5, 300.0)
    seen = {}
    for on in (True, False):
        gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=True, node_name="n", collective_slack=on)
        rings = be.make_rings(RANKS, 4, 256)
        try:
            srows = {"step": rings.row_for(0, "step")}
            krows = {GEMM: rings.row_for(1, GEMM)}  # (the all-reduce is in the rings' table only: the second report is the one-call one)
            rings.row_for(1, ALLREDUCE)
            for i in range(2):  # (stepwise, then one-call)
                for lr in range(RANKS):
                    rings.push_many(0, step, lr=lr)
                    rings.push_many(1, gemm, lr=lr)
                    rings.push_many(2, coll[lr], lr=lr)
                rep = gen.generate_report_from_rings(rings, srows, krows, local_ranks=RANKS)
                rings.reset()
                ws = gen._ring_plan.ws
                assert (rep.slack_scores() != {}) == on and gen._last_plan_fused == (i == 1)
                be.synchronize()
                seen[on, i] = (ws.stats_dev.cpu().numpy().tobytes(), ws.table.cpu().numpy().tobytes(),
                               dict(rep.gpu_relative_perf_scores), repr(rep.local_kernel_summaries))
        finally:
            gen.close()
            rings.close()
    for i in range(2):
        assert seen[True, i] == seen[False, i], i


@pytest.mark.parametrize("gather_on_rank0", [True, False])
def test_three_processes_sharing_the_gpu(gather_on_rank0):
    res = run_ranks(slack_workers.gpu_rank_late, 3, timeout=300, use_oracle_backend=False, device=0,
                    gather_on_rank0=gather_on_rank0)  # (returning at all: every rank finished)
    for r, reports in enumerate(res):
        for entry in reports:
            if gather_on_rank0 and r != 0:
                assert not entry["held"]
                continue
            s = entry["slack"]
            assert entry["flagged"] == [] and s["ranks_with_data"] == 3 and s["min_ranks"] == 3
            assert sorted(s["ranks"]) == ([0, 1, 2] if gather_on_rank0 else [r])
            # a report names among the ranks it covers: rank 0's with the gather, rank 1's own without
            assert entry["named"] == ([1] if (gather_on_rank0 or r == 1) else []), (r, entry)
            # (per call 300 us plus the difference of two exponential skews of 20 us, averaged over 200 calls: sigma 2 us)
            assert 290.0 * CALLS <= s["typical_waited_us"] <= 310.0 * CALLS
            if 1 in s["ranks"]:
                assert s["ranks"][1]["waited_us"] == 0.0


# ---- 4. per-kernel mode: dispatches with RCCL-like names reach their columns ---------------------------------------------------
def test_fed_collective_dispatches_reach_their_columns():
    import test_ktrace_datapath as cpu_twin
    from nvrx_straggler import ktrace
    from nvrx_straggler.reporting import ReportGenerator

    cap, per_key = 32, 20
    rng = np.random.default_rng(9)
    names = ["_Z17rcclGenericKernelILi1ELb0EEv24ncclDevKernelArgsStorageILm4096EE", "_Z21ncclDevKernel_AllGatherP11ncclDevComm",
             "_Z11mscclKernelILi2EEv", "_Z9gemm_tileILi128EEvPf", "_Z4reluPf"]
    ids = cpu_twin._fresh_kernel_ids(len(names))
    for i, n in zip(ids.tolist(), names):
        ktrace.feed_kernel_name(i, n)
    idx, dur, start, blocks = cpu_twin._launches(rng, names, per_key)
    disp = cpu_twin._as_dispatches(ids, idx, dur, start, blocks)
    ktrace.KernelTraceProfiler._live = None
    prof = ktrace.KernelTraceProfiler(statsMaxLenPerKernel=cap, max_keys=16)
    gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=True, node_name="n", collective_slack=True, slack_min_ranks=1)
    try:
        ktrace.feed(disp)
        assert prof.harvest(wait=True) == 0
        rings = prof._rings
        krows = prof.active_rows()
        assert len(krows) == len(names)
        srows = {"step": rings.row_for(0, "step")}
        rings.push_many(srows["step"], [1000.0] * 4)
        key_of = {k: next(key for key in krows if key.startswith(n + "_blk_")) for k, n in enumerate(names)}
        rep = gen.generate_report_from_rings(rings, srows, krows)
        s = rep.slack_scores()
        want = {}
        for k in range(3):  # the three collective kernels, by column
            us = (dur[idx == k].astype(np.float32) / np.float32(1000.0)).astype(np.float64)
            c = column_of(key_of[k])
            calls, total = want.get(c, (0, 0.0))
            want[c] = (calls + us.size, total + float(us.sum()))
        assert sorted(s["columns"]) == sorted(want) and s["ranks_with_data"] == 1 and sorted(s["ranks"]) == [0]
        for c, entry in s["columns"].items():
            assert entry["ranks"] == 1 and sorted(entry["kernels"]) == sorted(key_of[k] for k in range(3) if column_of(key_of[k]) == c)
        rec = s["ranks"][0]
        assert rec["calls"] == sum(v[0] for v in want.values()) == 3 * per_key
        total = sum(v[1] for v in want.values())
        assert abs(rec["collective_us"] - total) <= 2e-6 * total, (rec["collective_us"], total)
        compute = sum(float((dur[idx == k].astype(np.float32) / np.float32(1000.0)).astype(np.float64).sum()) for k in (3, 4))
        assert abs(rec["compute_us"] - compute) <= 2e-6 * compute
        assert rec["waited_us"] == 0.0 and rec["share"] == 0.0 and s["typical_waited_us"] == 0.0  # one rank waits for nobody
        assert named(rep.identify_slack_stragglers()) == []
        assert set(rep.local_kernel_summaries) == {key_of[3], key_of[4]}  # the report itself still drops the collective rows
    finally:
        gen.close()
        prof.close()
        ktrace.KernelTraceProfiler._live = None
