"""GPU parity of the pace-score kernels (``k_pace_cols`` in its three forms, ``k_pace_rank`` in its three) and of the pace
step of a report against the NumPy restatement of tests/pace_oracle_backend.py.  Every column and every rank of every case is
compared.

Bounds: column records, ``pace``, ``spread`` and all counts bit for bit (actual values; one f64 quotient rounded to f32 and one
f32 subtraction); a NaN the arithmetic itself makes (a spread of inf - inf) by NaN-ness only.  The three sums within
2e-6 * max(1, sum of |terms|): the tolerance tests/test_gpu_robust.py uses for an f64 weighted sum taken in another order,
relative to the sum of magnitudes because ``excess_us`` cancels; a sum that is not finite (a weight times 1 - inf) must be
the same kind of non-finite.

Shapes (R, K, S) sit at the geometry's edges: R 64 | 65 and 1024 | 1025 (``k_pace_cols``: tile, 256 threads, 1024 threads), a
part of 64 | 65 and 4096 | 4097 columns (``k_pace_rank``: one wave, keys in registers, re-reading)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import pace_workers
from mp_util import run_ranks
from pace_oracle_backend import pace_scores_table
from score_cases import random_table

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 3, 0), (2, 2, 2), (4, 0, 7), (8, 1, 1), (8, 63, 3), (8, 64, 0), (8, 65, 2), (64, 17, 33), (65, 70, 5),
          (3, 4096, 1), (3, 4097, 0), (100, 7, 9), (5, 3, 64), (5, 3, 65), (1024, 2, 1), (1025, 1, 2),
          (8, 300, 0), (8, 4096, 1), (8, 4097, 0)]  # (parts wider than a workgroup, with ranks enough for min_ranks = 4)
COLUMN_KINDS = ("zero_inf", "zero_zero", "equal", "equal", "equal", "below_min")
NAN_BITS = 0x7FC00000


@pytest.fixture(scope="module")
def be():
    from nvrx_straggler.backend import get_backend

    return get_backend()


def _special_column(T, rng, c, kind, K, S):
    R, KS = T.shape[0], K + S
    col = rng.lognormal(1.0, 0.5, R).astype(np.float32)
    col[rng.random(R) < 0.15] = -1.0
    if kind == "zero_inf":  # a 0.0 and a +inf among ordinary values: quotients of +inf and 0
        col[0] = 0.0
        col[R - 1] = np.inf if R > 1 else 0.0
    elif kind == "zero_zero":  # more than half the ranks hold 0: ctr = 0, and v = ctr = 0 is a NaN quotient
        col[rng.permutation(R)[: R // 2 + 1]] = 0.0
    elif kind == "equal":  # the same value on every rank: a quotient of exactly 1, repeated across a rank's median position
        col[:] = np.float32(3.25)
    elif kind == "below_min":  # present on three ranks at most: no reference at min_ranks = 4
        col[:] = -1.0
        col[rng.permutation(R)[:3]] = rng.lognormal(1.0, 0.5, min(3, R)).astype(np.float32)
    T[:, c] = col
    if c < K:
        T[:, 2 * KS + c] = np.where(col >= 0, rng.uniform(1, 1000, R), 0.0).astype(np.float32)


def _special_ranks(T, K, S):
    """Where at least four ranks keep their random values (R >= 7): the last rank eligible in no column, the one before it in
    a single column, and rank 1 AT the job's median in every column (every quotient 1: spread 0); a value equal to the lower
    median of the others leaves that median where it is."""
    R, KS = T.shape[0], K + S
    if R >= 7:
        T[R - 1, :KS] = -1.0
        T[R - 1, 2 * KS : 2 * KS + K] = 0.0
        keep = KS // 2
        T[R - 2, :keep], T[R - 2, keep + 1 : KS] = -1.0, -1.0
        T[R - 2, keep] = 2.5
        T[R - 2, 2 * KS : 2 * KS + K] = 0.0
        if keep < K:
            T[R - 2, 2 * KS + keep] = 40.0
        T[1, :KS] = -1.0
        ctr = pace_scores_table(T, K, S, 0, 1, 1)[0][:, 0].copy().view(np.float32)
        T[1, :KS] = np.where(np.isnan(ctr), -1.0, ctr)
        T[1, 2 * KS : 2 * KS + K] = np.where(T[1, :K] >= 0, 7.0, 0.0)


def _tables(R, K, S):
    """The tables of one case: ``random_table`` with 15 % of the medians absent, every rank scaled to a pace of its own, plus
    the special columns, spread over the columns (a case with fewer columns than kinds gets several tables), plus the
    special ranks."""
    rng = np.random.default_rng(R * 1000 + K + S)
    KS = K + S
    todo = list(COLUMN_KINDS)
    while todo:
        T = random_table(rng, R, K, S)
        # every rank at a pace of its own (0.7 x to 1.4 x): with identically distributed ranks a rank is AT the job's median in
        # so many columns that nearly every pace is the tie at exactly 1
        T[:, :KS] = np.where(T[:, :KS] >= 0, T[:, :KS] * rng.permutation(np.linspace(0.7, 1.4, R).astype(np.float32))[:, None], T[:, :KS])
        take, todo = todo[:KS], todo[KS:]
        cols = np.linspace(0, KS - 1, len(take)).astype(int) if len(take) > 1 else [KS // 2]
        for c, kind in zip(cols, take):
            _special_column(T, rng, int(c), kind, K, S)
        _special_ranks(T, K, S)
        yield T


def _run(be, T, K, S, first_rank, n_ranks, min_ranks):
    R = T.shape[0]
    ws = be.workspace(R, K, S, R, 0)
    ws.pace_settle()
    ws.send.copy_(torch.from_numpy(T))
    torch.cuda.synchronize()
    return be.pace_score(ws, ws.send, first_rank, n_ranks, min_ranks).records()


def _compare(got, exp, tag):
    (gcols, grecs), (ecols, erecs, terms) = got, exp
    assert gcols.shape == ecols.shape and grecs.shape == erecs.shape, tag
    bad = np.flatnonzero((gcols != ecols).any(axis=1))
    assert bad.size == 0, (tag, "columns", bad[:8].tolist(), gcols[bad[:4]], ecols[bad[:4]])
    # pace and the counts: bit for bit (a pace is a quotient that is not NaN, or the canonical NaN the kernel writes itself)
    exact = [0, 2, 3, 4]
    bad = np.argwhere(grecs[:, :, exact] != erecs[:, :, exact])
    assert bad.size == 0, (tag, "pace / counts", bad[:8].tolist(), grecs[tuple(bad[0][:2])], erecs[tuple(bad[0][:2])])
    # spread: bit for bit, except that inf - inf is a NaN of the arithmetic's own making
    gs, es = grecs[:, :, 1], erecs[:, :, 1]
    made = np.isnan(es.view(np.float32)) & (erecs[:, :, 0] != NAN_BITS)
    assert np.array_equal(np.isnan(gs.view(np.float32)), np.isnan(es.view(np.float32))), (tag, "spread NaN masks")
    bad = np.argwhere((gs != es) & ~made)
    assert bad.size == 0, (tag, "spread", bad[:8].tolist(), gs[tuple(bad.T)][:8], es[tuple(bad.T)][:8])
    # the sums: part 1 is +0.0; part 0 within the tolerance of a sum taken in another order
    assert (grecs[:, 1, 5:] == 0).all(), (tag, "section sums")
    g, e = grecs[:, 0, 5:].view(np.float32).astype(np.float64), erecs[:, 0, 5:].view(np.float32).astype(np.float64)
    fin = np.isfinite(e)
    assert np.array_equal(np.isnan(g), np.isnan(e)) and np.array_equal(np.isposinf(g), np.isposinf(e)) and \
        np.array_equal(np.isneginf(g), np.isneginf(e)), (tag, "non-finite sums", g[~fin], e[~fin])
    if fin.any():
        err = np.abs(g[fin] - e[fin]) / np.maximum(1.0, terms[fin])
        print(tag, "sums: max error", float(err.max()), "of", int(fin.sum()))
        assert err.max() <= 2e-6, (tag, "sums", float(err.max()))


@pytest.mark.parametrize("R,K,S", SHAPES)
def test_pace_score_matches_numpy(be, R, K, S):
    seen_single = seen_none = seen_flat = False
    for t, T in enumerate(_tables(R, K, S)):
        for min_ranks in (1, 4):
            tag = (R, K, S, t, min_ranks)
            got = _run(be, T, K, S, 0, R, min_ranks)
            exp = pace_scores_table(T, K, S, 0, R, min_ranks)
            _compare(got, exp, tag)
            recs = exp[1]
            if max(K, S) > 64 and (min_ranks == 1 or R >= 4):
                # the selections of a wide part get something to select from: the ranks' spreads differ, and so do their
                # paces (with few ranks a good part of a rank's quotients are exactly 1, and the median falls among those ties)
                p = 0 if K >= S else 1
                live = recs[:, p, 0] != NAN_BITS
                assert np.unique(recs[live & (recs[:, p, 1] != 0), p, 1]).size >= 2, (tag, recs[:, p, :2])
                assert R < 7 or np.unique(recs[live, p, 0]).size >= 3, (tag, recs[:, p, :2])
            if R >= 7 and min_ranks == 1:
                # the special ranks are what they were built to be
                assert (recs[R - 1, :, 2:5] == 0).all() and (recs[R - 1, :, :2] == NAN_BITS).all(), tag
                assert recs[R - 2, :, 2].sum() <= 1, tag
                seen_none = True
                seen_single = seen_single or recs[R - 2, :, 2].sum() == 1
                for p in range(2):
                    if recs[1, p, 2]:
                        assert recs[1, p, 3] == 0 and recs[1, p, 4] == 0, tag  # neither slower nor faster than the median
                        f = recs[1, p, :2].view(np.float32)
                        if f[0] == 1.0:
                            assert f[1] == 0.0, tag
                            seen_flat = True
        # a sub-range of ranks equals the slice of the full result, bit for bit (the same workgroups do the same sums)
        lo, n = (R // 3, max(1, R // 2)) if R > 1 else (0, 1)
        pcols, precs = _run(be, T, K, S, lo, n, 4)
        assert np.array_equal(pcols, got[0]) and np.array_equal(precs, got[1][lo : lo + n]), (R, K, S, t, "sub-range")
    if R >= 7:
        assert seen_none and seen_single and seen_flat, (R, K, S)


def test_nothing_is_written_outside_the_records(be):
    from nvrx_straggler import _native

    PAD, FILL = 64, 0x5A5A5A5A
    rng = np.random.default_rng(78)
    for R, K, S, first, n in ((9, 5, 70, 0, 9), (9, 5, 70, 4, 3), (70, 66, 3, 60, 10), (3, 4100, 2, 1, 2)):
        T = random_table(rng, R, K, S)
        table = torch.from_numpy(T).cuda()
        words = _native.pace_words(n, K, S)
        out = torch.full((PAD + words + PAD,), FILL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        rc = be.lib.nvrx_pace_score(table.data_ptr(), R, K, S, first, n, 2, out.data_ptr() + 4 * PAD, be._stream_handle)
        assert rc == 0, be.lib.nvrx_last_error()
        be.synchronize()
        torch.cuda.synchronize()
        host = out.cpu().numpy().view(np.uint32)
        assert (host[:PAD] == FILL).all() and (host[PAD + words :] == FILL).all(), (R, K, S)
        body = host[PAD : PAD + words]
        KS = K + S
        _compare((body[: 4 * KS].reshape(KS, 4), body[4 * KS :].reshape(n, 2, 8)), pace_scores_table(T, K, S, first, n, 2),
                 (R, K, S, first, n))


def test_argument_errors_come_back_before_the_device_is_touched(be):
    import ctypes

    from nvrx_straggler import _native

    lib = be.lib
    R, K, S = 8, 8, 2
    table = torch.zeros((R, _native.table_len(K, S)), dtype=torch.float32, device="cuda")
    out = torch.full((_native.pace_words(R, K, S),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def score(tp=table.data_ptr(), R=R, first=0, n=R, min_ranks=4, op=out.data_ptr()):
        return lib.nvrx_pace_score(tp, R, K, S, first, n, min_ranks, op, be._stream_handle)

    assert score(tp=None) == _native.ERR_INVALID and score(op=None) == _native.ERR_INVALID
    assert score(R=_native.ROBUST_MAX_RANKS + 1, n=1) == _native.ERR_RANGE
    assert score(first=7, n=2) == _native.ERR_RANGE and score(first=-1) == _native.ERR_RANGE and score(n=R + 1) == _native.ERR_RANGE
    assert score(min_ranks=0) == _native.ERR_RANGE
    assert score(op=out.data_ptr() + 4) == _native.ERR_INVALID
    desc = _native.ReportDesc()
    desc.R, desc.K, desc.S = R, K, S
    assert lib.nvrx_report_pace(None, ctypes.byref(desc), 0, R, 4, out.data_ptr()) == _native.ERR_INVALID
    rings = be.make_rings(1, 4, 16)
    try:  # a context no report went through this descriptor on
        assert lib.nvrx_report_pace(rings.ctx, ctypes.byref(desc), 0, R, 4, out.data_ptr()) == _native.ERR_STATE
    finally:
        rings.close()
    be.synchronize()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x5A5A5A5A).all()  # nothing was launched


# ---- the pace step of a report --------------------------------------------------------------------------------------------
def _same_as_direct(rep, tag):
    """What the report's pace step wrote IS what ``nvrx_pace_score`` says of the same table (same kernels, same order of
    sums: every word equal), and both are what the restatement says of it."""
    R, K, S = rep["shape"]
    t = rep["pace"]
    cols, recs = rep["direct"]
    _compare((cols, recs), pace_scores_table(rep["table"], K, S, 0, R, t["params"]["min_ranks"]), tag)
    f = recs.view(np.float32)
    for r in range(R):
        for p, part in enumerate(("gpu", "sections")):
            d = t["ranks"][r][part]
            assert [d["columns"], d["slower"], d["faster"]] == recs[r, p, 2:5].tolist(), (tag, r, part)
            assert d["pace"] == float(f[r, p, 0]) and d["spread"] == float(f[r, p, 1]), (tag, r, part)
        gpu = t["ranks"][r]["gpu"]
        assert [gpu["total_us"], gpu["slower_us"], gpu["excess_us"]] == f[r, 0, 5:].tolist(), (tag, r)
    shown = sorted((c["center"], c["ranks"], c["above"], c["below"]) for c in list(t["kernels"].values()) + list(t["section_columns"].values()))
    assert shown == sorted((float(c), int(n), int(a), int(b)) for c, (n, a, b) in zip(cols[:, 0].copy().view(np.float32), cols[:, 1:])), tag


def _check_reports(reports, fused_want):
    assert [r["fused"] for r in reports] == fused_want
    compared = 0
    for i, rep in enumerate(reports):
        assert rep["named"] == [pace_workers.SLOW_RANK] and rep["job_named"] == [] and rep["robust_named"] == [], (i, rep["named"])
        t = rep["pace"]
        assert sorted(t["ranks"]) == list(range(8)) and sorted(t["kernels"]) == sorted(pace_workers.KERNEL_NAMES)
        assert t["ranks"][5]["gpu"]["slower"] == 120 and t["ranks"][5]["gpu"]["columns"] == 120
        if "direct" not in rep:
            continue
        compared += 1
        assert rep["shape"] == (8, 120, 1)
        _same_as_direct(rep, ("report", i))
    assert compared >= 2


@pytest.mark.parametrize("asynchronous", [False, True])
def test_report_step_on_the_general_and_the_one_call_path(be, asynchronous):
    _check_reports(pace_workers.folded_pace(0, 1, asynchronous=asynchronous), [False, True, True])


def test_report_step_behind_a_report_that_was_scored_resident():
    """``nvrx_report_pace``'s ordering: the score kernel ran on a stream of its own, the pace kernels follow it by an event."""
    res = run_ranks(pace_workers.folded_pace_sync_then_async, 1, timeout=300, use_oracle_backend=False, device=0,
                    env={"NVRX_DEBUG_RESIDENT_SCORER": "2"})[0]
    for mode in ("sync", "async"):
        _check_reports(res[mode], [False, True, True])


def test_report_step_behind_reports_that_were_rehomed():
    """Asynchronous Detector reports re-homed onto the stream of their stamps: every report's pace step read its own window,
    and wrote what ``nvrx_pace_score`` says of that window's table."""
    res = run_ranks(pace_workers.detector_rehomed, 1, timeout=300, use_oracle_backend=False, device=0,
                    env={"NVRX_DEBUG_ASYNC_REHOME_GAP_US": "1"})[0]
    assert res["rehomed"] > 0 and res["lane_is_none"]
    compared = 0
    for t, rep in enumerate(res["reports"], start=1):
        scores = rep["pace"]
        for i in range(3):
            assert scores["section_columns"][f"s{i}"] == {"center": float(10 * t + i), "ranks": 1, "above": 0, "below": 0}, (t, i)
        assert scores["ranks"][0]["sections"] == {"pace": 1.0, "spread": 0.0, "columns": 3, "slower": 0, "faster": 0, "breadth": 0.0}
        assert scores["ranks"][0]["gpu"]["pace"] == 1.0 and scores["ranks"][0]["gpu"]["columns"] == 3
        if "direct" in rep:
            compared += 1
            assert rep["shape"][0] == 1 and rep["shape"][1] >= 3 and rep["shape"][2] >= 3, rep["shape"]
            _same_as_direct(rep, ("re-homed", t))
    assert compared >= len(res["reports"]) - 1


def test_a_report_held_across_the_next_two_is_still_its_own():
    out = pace_workers.held_reports(0, 1)
    assert len(out) == 5
    for w, t in enumerate(out):
        # four ranks at 10 (w + 1) + {0, 1, 2, 3}: the lower median is rank 1's
        assert t["kernels"]["gemm"] == {"center": 10.0 * (w + 1) + 1.0, "ranks": 4, "above": 2, "below": 1}, (w, t["kernels"])
        assert t["section_columns"]["step"]["center"] == 100.0 * (w + 1) + 1.0
        assert t["ranks"][3]["gpu"]["pace"] == float(np.float32((10.0 * (w + 1) + 1.0) / (10.0 * (w + 1) + 3.0)))


def test_the_example_names_rank_5_alone():
    out = subprocess.run([sys.executable, os.path.join(REPO, "examples", "straggler_example.py"), "--pace"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    found = {name: re.search(name + r"\(\): (\[[^\]]*\])", out.stdout) for name in
             ("identify_stragglers", "identify_robust_stragglers", "identify_pace_stragglers")}
    assert all(found.values()), out.stdout
    assert found["identify_stragglers"].group(1) == "[]" and found["identify_robust_stragglers"].group(1) == "[]", out.stdout
    assert found["identify_pace_stragglers"].group(1) == "[5]", out.stdout
