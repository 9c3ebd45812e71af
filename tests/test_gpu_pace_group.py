"""GPU parity of the kernels of pace scores per peer group (``k_pace_group_cols`` in its three forms, ``k_pace_rank`` in its
three grouped instantiations) and of the grouped pace step of a report against the NumPy restatement of
tests/pace_group_oracle_backend.py.  Every pair of group and column and every rank of every case is compared.

Bounds: column records, ``pace``, ``spread`` and all counts bit for bit (actual values; one f64 quotient rounded to f32 and one
f32 subtraction); a NaN the arithmetic itself makes (a spread of inf - inf) by NaN-ness only.  The three sums within
2e-6 * max(1, sum of |terms|): the tolerance tests/test_gpu_pace.py uses for an f64 weighted sum taken in another order,
relative to the sum of magnitudes because ``excess_us`` cancels; a sum that is not finite must be the same kind of non-finite.

Shapes (R, K, S) and groupings sit at the geometry's edges: the 64-column tile of the tiled columns kernel, a largest group of
64 | 65 and 1024 | 1025 members (tiled, 256 threads, 1024 threads), a part of 64 | 65 and 4096 | 4097 columns (the rank
kernel: one wave, keys in registers, re-reading).  Memberships are mostly NOT contiguous (``mod:N``, random labels, interleaved
groups): a kernel that reads row ``s + i`` instead of ``members[s + i]`` passes every ``block:N`` case."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import pace_group_workers as workers
from mp_util import run_ranks
from pace_group_oracle_backend import pace_group_scores_table, threshold
from pace_oracle_backend import pace_scores_table
from score_cases import random_table

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(1, 3, 0, "one"), (2, 2, 2, "one"), (2, 2, 2, "singletons"), (8, 1, 1, "block:4"), (8, 1, 1, "mod:2"),
         (8, 1, 1, "random:3"), (8, 63, 3, "mod:2"), (8, 64, 0, "mod:2"), (8, 65, 2, "mod:2"), (4, 4097, 0, "block:2"),
         (64, 17, 33, "one"), (64, 17, 33, "block:16"), (65, 70, 5, "mod:2"), (65, 70, 5, "one"), (100, 7, 9, "65+35"),
         (1025, 3, 2, "one"), (1025, 3, 2, "mod:17")]
COLUMN_KINDS = ("absent_in_group", "only_in_group", "nan_inf_zero", "equal", "ties", "at_threshold", "below_threshold")
NAN_BITS = 0x7FC00000


@pytest.fixture(scope="module")
def be():
    from nvrx_straggler.backend import get_backend

    return get_backend()


def _labels(R, grouping):
    kind, _, num = grouping.partition(":")
    if kind == "one":
        return [0] * R
    if kind == "singletons":
        return list(range(R))
    if kind == "block":
        return [r // int(num) for r in range(R)]
    if kind == "mod":
        return [r % int(num) for r in range(R)]
    if kind == "random":
        return np.random.default_rng(R).integers(0, int(num), R).tolist()
    assert grouping == "65+35" and R == 100
    labels = np.zeros(R, dtype=int)
    labels[np.linspace(1, 98, 35).astype(int)] = 1  # 35 ranks spread among the other 65
    assert labels.sum() == 35
    return labels.tolist()


def _special_column(T, rng, c, kind, K, S, members):
    """One column made special WITHIN one group (``members``); the other groups keep ordinary values."""
    R, KS = T.shape[0], K + S
    n = len(members)
    col = rng.lognormal(1.0, 0.5, R).astype(np.float32)
    col[rng.random(R) < 0.15] = -1.0
    need = threshold(4, 2, n)
    if kind == "absent_in_group":
        col[members] = -1.0
    elif kind == "only_in_group":
        mine = col[members]
        col[:] = -1.0
        col[members] = np.abs(mine)
    elif kind == "nan_inf_zero":  # quotients of +inf and 0, and a NaN that is absent
        col[members] = rng.lognormal(1.0, 0.5, n).astype(np.float32)
        col[members[0]] = 0.0
        col[members[-1]] = np.inf if n > 1 else 0.0
        if n > 2:
            col[members[n // 2]] = np.nan
    elif kind == "equal":  # the same value on every member: quotients of exactly 1
        col[members] = np.float32(3.25)
    elif kind == "ties":  # most members hold the median's value
        col[members] = rng.choice(np.array([1.5, 2.0, 2.0, 2.0, 2.5], dtype=np.float32), n)
    elif kind in ("at_threshold", "below_threshold"):  # exactly as many present members as a reference needs, and one fewer
        keep = min(n, need if kind == "at_threshold" else need - 1)
        col[members] = -1.0
        col[rng.permutation(members)[:keep]] = rng.lognormal(1.0, 0.5, keep).astype(np.float32)
    T[:, c] = col
    if c < K:
        with np.errstate(invalid="ignore"):
            T[:, 2 * KS + c] = np.where(col >= 0, rng.uniform(1, 1000, R), 0.0).astype(np.float32)


def _tables(R, K, S, labels):
    """The tables of one case: ``random_table`` with 15 % of the medians absent, every rank scaled to a pace of its own, plus
    the special columns, each within one group in turn, spread over the columns (a case with fewer columns than kinds gets
    several tables)."""
    rng = np.random.default_rng(R * 1000 + K + S)
    KS = K + S
    labels = np.asarray(labels)
    G = int(labels.max()) + 1
    todo = list(enumerate(COLUMN_KINDS))
    while todo:
        T = random_table(rng, R, K, S)
        T[:, :KS] = np.where(T[:, :KS] >= 0, T[:, :KS] * rng.permutation(np.linspace(0.7, 1.4, R).astype(np.float32))[:, None], T[:, :KS])
        take, todo = todo[:KS], todo[KS:]
        cols = np.linspace(0, KS - 1, len(take)).astype(int) if len(take) > 1 else [KS // 2]
        for c, (j, kind) in zip(cols, take):
            _special_column(T, rng, int(c), kind, K, S, np.flatnonzero(labels == j % G))
        yield T


def _run(be, T, K, S, groups, first_rank, n_ranks, min_ranks, min_peers):
    R = T.shape[0]
    ws = be.workspace(R, K, S, R, 0)
    ws.pace_settle()
    ws.send.copy_(torch.from_numpy(T))
    torch.cuda.synchronize()
    return be.pace_group_score(ws, ws.send, groups, first_rank, n_ranks, min_ranks, min_peers).records()


def _compare(got, exp, tag):
    (gcols, grecs), (ecols, erecs, terms) = got, exp
    assert gcols.shape == ecols.shape and grecs.shape == erecs.shape, tag
    gcols, ecols = gcols.reshape(-1, 4), ecols.reshape(-1, 4)
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


@pytest.mark.parametrize("R,K,S,grouping", CASES)
def test_pace_group_score_matches_numpy(be, R, K, S, grouping):
    from nvrx_straggler.backend import PeerGroups

    labels = _labels(R, grouping)
    groups = PeerGroups(labels)
    G, largest = groups.G, groups.max_size
    rated = unreferenced = False
    for t, T in enumerate(_tables(R, K, S, labels)):
        for min_ranks, min_peers in ((4, 2), (1, 1)):
            tag = (R, K, S, grouping, t, min_ranks, min_peers)
            got = _run(be, T, K, S, groups, 0, R, min_ranks, min_peers)
            exp = pace_group_scores_table(T, K, S, groups.host, G, largest, 0, R, min_ranks, min_peers)
            _compare(got, exp, tag)
            rated = rated or bool((exp[1][:, :, 2] > 0).any())
            unreferenced = unreferenced or bool(((exp[0][:, :, 0] == NAN_BITS) & (exp[0][:, :, 1] > 0)).any())
        # a window of ranks that starts and ends inside a group equals the slice of the full result, bit for bit
        lo, n = (R // 3, max(1, R // 2)) if R > 1 else (0, 1)
        pcols, precs = _run(be, T, K, S, groups, lo, n, 1, 1)
        assert np.array_equal(pcols, got[0]) and np.array_equal(precs, got[1][lo : lo + n]), (R, K, S, grouping, t, "window")
    assert rated, (R, K, S, grouping)  # the case rates somebody ...
    assert unreferenced or R == 1, (R, K, S, grouping)  # ... and has pairs with data and no reference


@pytest.mark.parametrize("R,K,S", [(8, 65, 2), (64, 17, 33), (65, 70, 5), (3, 4097, 0), (1025, 3, 2)])
def test_one_group_and_one_peer_minimum_is_the_job_wide_pace_score(be, R, K, S):
    """Both entry points on the same table: column and rank records bit for bit except the three sums (two instantiations of
    the rank kernel need not add in one order), which get the bound above."""
    from nvrx_straggler.backend import PeerGroups

    groups = PeerGroups([0] * R)
    for t, T in enumerate(_tables(R, K, S, [0] * R)):
        for min_ranks in (1, min(4, R)):
            grouped = _run(be, T, K, S, groups, 0, R, min_ranks, 1)
            ws = be.workspace(R, K, S, R, 0)
            cols, recs = be.pace_score(ws, ws.send, 0, R, min_ranks).records()
            terms = pace_scores_table(T, K, S, 0, R, min_ranks)[2]
            assert grouped[0].shape == (1, K + S, 4)
            _compare(grouped, (cols[None], recs, terms), (R, K, S, t, min_ranks))


def test_out_of_range_group_contents_are_guarded(be):
    """Group ids outside [0, G), members outside [0, R), ``start`` words negative, decreasing and beyond R, and a stretch above
    ``max_group``: the result is what the restatement says, and no word outside NVRX_PACE_GROUP_WORDS of a guard-padded buffer
    is touched.  Valid launches only: the kernels' guards keep every access inside the table, the array and the buffer."""
    from nvrx_straggler import _native
    from nvrx_straggler.backend import PeerGroups

    PAD, FILL = 64, 0x5A5A5A5A
    rng = np.random.default_rng(79)
    # the tiled kernel (groups of 5 or 6, once cut to 4), and the 256-thread one (groups of 66 and 4, cut to 65)
    for R, K, S, labels, largest in ((21, 5, 70, [r % 4 for r in range(21)], 6), (21, 5, 70, [r % 4 for r in range(21)], 4),
                                     (70, 66, 3, [1 if r % 17 == 3 else 0 for r in range(70)], 65)):
        G = max(labels) + 1
        T = random_table(rng, R, K, S)
        good = PeerGroups(labels).host
        cases = {"intact": good.copy()}
        a = cases["group id G and -1"] = good.copy()
        a[3], a[8] = G, -1
        a = cases["member R and -1"] = good.copy()
        a[R + 2], a[R + 9] = R, -1
        a = cases["start beyond R"] = good.copy()
        a[2 * R + G] = R + 5
        a = cases["start below 0 and descending"] = good.copy()
        a[2 * R], a[2 * R + 1] = -3, 0
        if G > 2:
            a[2 * R + 2] = 1
        a = cases["everything"] = good.copy()
        a[0], a[R + R - 1], a[2 * R + G], a[2 * R + 1] = G + 7, 1 << 30, 1 << 30, -(1 << 30)
        table = torch.from_numpy(T).cuda()
        for name, arrays in cases.items():
            for first, n in ((0, R), (4, 9)):
                words = _native.pace_group_words(G, n, K, S)
                out = torch.full((PAD + words + PAD,), FILL, dtype=torch.int32, device="cuda")
                d_groups = torch.from_numpy(arrays).cuda()
                torch.cuda.synchronize()
                rc = be.lib.nvrx_pace_group_score(table.data_ptr(), R, K, S, d_groups.data_ptr(), G, largest, first, n, 4, 2,
                                                  out.data_ptr() + 4 * PAD, be._stream_handle)
                assert rc == 0, (name, be.lib.nvrx_last_error())
                be.synchronize()
                torch.cuda.synchronize()
                host = out.cpu().numpy().view(np.uint32)
                assert (host[:PAD] == FILL).all() and (host[PAD + words :] == FILL).all(), (R, name)
                body = host[PAD : PAD + words]
                KS = K + S
                got = (body[: 4 * G * KS].reshape(G, KS, 4), body[4 * G * KS :].reshape(n, 2, 8))
                _compare(got, pace_group_scores_table(T, K, S, arrays, G, largest, first, n, 4, 2), (R, largest, name, first, n))
                if name == "group id G and -1" and first == 0:
                    assert (got[1][[3, 8], :, 2:] == 0).all() and (got[1][[3, 8], :, :2] == NAN_BITS).all()
                    assert (got[1][4, :, 2] > 0).any()
                if name == "intact":
                    assert int(got[0][0, :, 1].max()) <= largest  # a stretch above max_group is cut


def test_argument_errors_come_back_before_the_device_is_touched(be):
    import ctypes

    from nvrx_straggler import _native
    from nvrx_straggler.backend import PeerGroups

    lib = be.lib
    R, K, S, G = 8, 8, 2, 2
    table = torch.zeros((R, _native.table_len(K, S)), dtype=torch.float32, device="cuda")
    out = torch.full((_native.pace_group_words(G, R, K, S),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    d_groups = torch.from_numpy(PeerGroups([r % G for r in range(R)]).host).cuda()
    torch.cuda.synchronize()

    def score(tp=table.data_ptr(), R=R, gp=d_groups.data_ptr(), G=G, largest=4, first=0, n=R, min_ranks=4, min_peers=2,
              op=out.data_ptr()):
        return lib.nvrx_pace_group_score(tp, R, K, S, gp, G, largest, first, n, min_ranks, min_peers, op, be._stream_handle)

    def said(text):
        return text in lib.nvrx_last_error().decode()

    assert score(tp=None) == _native.ERR_INVALID and score(gp=None) == _native.ERR_INVALID and score(op=None) == _native.ERR_INVALID
    assert score(R=_native.ROBUST_MAX_RANKS + 1, n=1) == _native.ERR_RANGE
    assert score(first=7, n=2) == _native.ERR_RANGE and score(first=-1) == _native.ERR_RANGE and score(n=R + 1) == _native.ERR_RANGE
    assert score(min_ranks=0) == _native.ERR_RANGE
    assert score(G=0) == _native.ERR_INVALID and score(G=R + 1) == _native.ERR_RANGE
    assert score(largest=0) == _native.ERR_RANGE and score(largest=R + 1) == _native.ERR_RANGE and score(min_peers=0) == _native.ERR_RANGE
    assert score(op=out.data_ptr() + 4) == _native.ERR_INVALID
    # the stated order: pace's checks, then G, then max_group and min_peers, then the pointers
    assert score(R=0, first=5, n=4, min_ranks=0, G=0, largest=0, min_peers=0, tp=None) == _native.ERR_INVALID and said("shape")
    assert score(first=5, n=4, min_ranks=0, G=0, largest=0, min_peers=0, tp=None) == _native.ERR_RANGE and said("outside")
    assert score(min_ranks=0, G=0, largest=0, min_peers=0, tp=None) == _native.ERR_RANGE and said("min_ranks")
    assert score(G=0, largest=0, min_peers=0, tp=None) == _native.ERR_INVALID and said("groups")
    assert score(G=R + 1, largest=0, min_peers=0, tp=None) == _native.ERR_RANGE and said("groups")
    assert score(largest=0, min_peers=0, tp=None) == _native.ERR_RANGE and said("max_group")
    assert score(min_peers=0, tp=None) == _native.ERR_RANGE and said("min_peers")
    desc = _native.ReportDesc()
    desc.R, desc.K, desc.S = R, K, S
    gp = d_groups.data_ptr()
    assert lib.nvrx_report_pace_group(None, ctypes.byref(desc), gp, G, 4, 0, R, 4, 2, out.data_ptr()) == _native.ERR_INVALID
    rings = be.make_rings(1, 4, 16)
    try:  # a context no report went through this descriptor on
        assert lib.nvrx_report_pace_group(rings.ctx, ctypes.byref(desc), gp, G, 9, 0, R, 4, 2, out.data_ptr()) == _native.ERR_RANGE
        assert lib.nvrx_report_pace_group(rings.ctx, ctypes.byref(desc), None, G, 4, 0, R, 4, 2, out.data_ptr()) == _native.ERR_INVALID
        assert lib.nvrx_report_pace_group(rings.ctx, ctypes.byref(desc), gp, G, 4, 0, R, 4, 2, out.data_ptr()) == _native.ERR_STATE
    finally:
        rings.close()
    be.synchronize()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x5A5A5A5A).all()  # nothing was launched


# ---- the grouped pace step of a report ------------------------------------------------------------------------------------
def _same_as_direct(rep, tag, min_ranks, min_peers):
    """What the report's pace step wrote IS what ``nvrx_pace_group_score`` says of the same table (same kernels, same order of
    sums: every word equal), and both are what the restatement says of it."""
    R, K, S = rep["shape"]
    t = rep["pace"]
    cols, recs = rep["direct"]
    host, G, largest = rep["groups"]
    _compare((cols, recs), pace_group_scores_table(rep["table"], K, S, host, G, largest, 0, R, min_ranks, min_peers), tag)
    assert t["params"]["min_ranks"] == min_ranks and t["params"]["min_peers"] == min_peers and t["params"]["peer_groups"] is True
    f = recs.view(np.float32)
    for r in range(R):
        for p, part in enumerate(("gpu", "sections")):
            d = t["ranks"][r][part]
            assert [d["columns"], d["slower"], d["faster"]] == recs[r, p, 2:5].tolist(), (tag, r, part)
            assert d["pace"] == float(f[r, p, 0]) and d["spread"] == float(f[r, p, 1]), (tag, r, part)
        gpu = t["ranks"][r]["gpu"]
        assert [gpu["total_us"], gpu["slower_us"], gpu["excess_us"]] == f[r, 0, 5:].tolist(), (tag, r)
    labels = list(t["groups"])
    shown = sorted((labels.index(g), x["center"], x["ranks"], x["above"], x["below"])
                   for c in list(t["kernels"].values()) + list(t["section_columns"].values()) for g, x in c.items())
    want = sorted((g, float(c), int(n), int(a), int(b)) for g in range(G)
                  for c, (n, a, b) in zip(cols[g, :, 0].copy().view(np.float32), cols[g, :, 1:]))
    assert shown == want, tag


def _check_reports(reports, fused_want):
    assert [r["fused"] for r in reports] == fused_want
    compared = 0
    for i, rep in enumerate(reports):
        assert rep["named"] == [workers.SLOW_RANK], (i, rep["named"])
        t = rep["pace"]
        assert sorted(t["ranks"]) == list(range(8)) and sorted(t["kernels"]) == sorted(workers.KERNEL_NAMES)
        assert t["groups"] == {0: [0, 1, 2, 3], 1: [4, 5, 6, 7]} and t["unrated_ranks"] == []
        assert t["ranks"][6]["gpu"]["slower"] == 120 and t["ranks"][6]["gpu"]["columns"] == 120
        assert all(t["ranks"][r]["gpu"]["breadth"] < 0.9 for r in range(8) if r != 6)
        if "direct" not in rep:
            continue
        compared += 1
        assert rep["shape"] == (8, 120, 1)
        _same_as_direct(rep, ("report", i), 4, 2)
    assert compared >= 2


@pytest.mark.parametrize("asynchronous", [False, True])
def test_report_step_on_the_general_and_the_one_call_path(be, asynchronous):
    _check_reports(workers.folded_pace_group(0, 1, asynchronous=asynchronous), [False, True, True])


def test_report_step_behind_a_report_that_was_scored_resident():
    """``nvrx_report_pace_group``'s ordering: the score kernel ran on a stream of its own, the pace kernels follow it by an
    event."""
    res = run_ranks(workers.folded_pace_group_sync_then_async, 1, timeout=300, use_oracle_backend=False, device=0,
                    env={"NVRX_DEBUG_RESIDENT_SCORER": "2"})[0]
    for mode in ("sync", "async"):
        _check_reports(res[mode], [False, True, True])


def test_report_step_behind_reports_that_were_rehomed():
    """Asynchronous Detector reports re-homed onto the stream of their stamps: every report's pace step read its own window,
    and wrote what ``nvrx_pace_group_score`` says of that window's table."""
    res = run_ranks(workers.detector_rehomed, 1, timeout=300, use_oracle_backend=False, device=0,
                    env={"NVRX_DEBUG_ASYNC_REHOME_GAP_US": "1"})[0]
    assert res["rehomed"] > 0 and res["lane_is_none"]
    compared = 0
    for t, rep in enumerate(res["reports"], start=1):
        scores = rep["pace"]
        for i in range(3):
            assert scores["section_columns"][f"s{i}"] == {0: {"center": float(10 * t + i), "ranks": 1, "above": 0, "below": 0}}, (t, i)
        assert scores["ranks"][0]["sections"] == {"pace": 1.0, "spread": 0.0, "columns": 3, "slower": 0, "faster": 0, "breadth": 0.0}
        assert scores["ranks"][0]["gpu"]["pace"] == 1.0 and scores["ranks"][0]["gpu"]["columns"] == 3
        assert scores["unrated_ranks"] == []
        if "direct" in rep:
            compared += 1
            assert rep["shape"][0] == 1 and rep["shape"][1] >= 3 and rep["shape"][2] >= 3, rep["shape"]
            _same_as_direct(rep, ("re-homed", t), 1, 1)
    assert compared >= len(res["reports"]) - 1


def test_a_report_held_across_the_next_two_is_still_its_own():
    out = workers.held_reports(0, 1)
    assert len(out) == 5
    for w, t in enumerate(out):
        # mod:2 -- ranks {0, 2} at 10 (w + 1) + {0, 2}, ranks {1, 3} at + {1, 3}: a group of two is rated against its faster member
        base = 10.0 * (w + 1)
        assert t["kernels"]["gemm"] == {0: {"center": base, "ranks": 2, "above": 1, "below": 0},
                                        1: {"center": base + 1.0, "ranks": 2, "above": 1, "below": 0}}, (w, t["kernels"])
        assert t["section_columns"]["step"][1]["center"] == 100.0 * (w + 1) + 1.0
        assert t["ranks"][3]["gpu"]["pace"] == float(np.float32((base + 1.0) / (base + 3.0)))
        assert t["ranks"][0]["gpu"]["pace"] == 1.0 and t["group_of"] == {0: 0, 1: 1, 2: 0, 3: 1}


def test_the_example_names_rank_6_alone_where_the_job_wide_rule_names_four():
    out = subprocess.run([sys.executable, os.path.join(REPO, "examples", "straggler_example.py"), "--pace-peer"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    found = re.findall(r"identify_pace_stragglers\(\) ([a-z-]+): (\[[^\]]*\])", out.stdout)
    assert found == [("job-wide", "[4, 5, 6, 7]"), ("per-peer-group", "[6]")], out.stdout
