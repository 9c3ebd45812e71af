"""GPU parity of the node-score kernels (``k_node_cols``, ``k_pace_group_cols`` + ``k_node_across`` in both forms, the NODE
instantiations of ``k_pace_rank``) and of the node step of a report against the NumPy restatement of
tests/node_oracle_backend.py.  Every pair, column, node and rank of every case is compared.

Bounds: blocks A, B and C and the exact words of D (``pace``, ``spread``, the counts) bit for bit -- actual values, one f64
quotient rounded to f32 and one f32 subtraction; a NaN the arithmetic itself makes (a spread of inf - inf) by NaN-ness only.
D's three sums within 2e-6 * max(1, sum of |terms|): the tolerance tests/test_gpu_pace_group.py uses for an f64 weighted sum
taken in another order, relative to the sum of magnitudes because ``excess_us`` cancels; a sum that is not finite must be the
same kind of non-finite.  C's sum slots are +0.0.

The cases, their tables and what each case must hold are tests/node_cases.py's; tests/test_node_host.py checks the latter on
the restatement alone."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import node_cases
import node_workers as workers
from mp_util import run_ranks
from node_cases import NAN_BITS
from node_oracle_backend import node_scores_table
from pace_oracle_backend import pace_scores_table
from score_cases import random_table

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def be():
    from nvrx_straggler.backend import get_backend

    return get_backend()


def _run(be, T, K, S, nodes, min_members, min_nodes, first_rank, n_ranks):
    R = T.shape[0]
    ws = be.workspace(R, K, S, R, 0)
    ws.node_settle()
    ws.pace_settle()
    ws.send.copy_(torch.from_numpy(T))
    torch.cuda.synchronize()
    return be.node_score(ws, ws.send, nodes, first_rank, n_ranks, min_members, min_nodes).records()


def _compare_exact(got, exp, tag, what):
    assert got.shape == exp.shape, (tag, what, got.shape, exp.shape)
    g, e = got.reshape(-1, got.shape[-1]), exp.reshape(-1, exp.shape[-1])
    bad = np.flatnonzero((g != e).any(axis=1))
    assert bad.size == 0, (tag, what, bad[:8].tolist(), g[bad[:4]], e[bad[:4]])


def _compare_records(grecs, erecs, tag, what):
    """pace and the counts bit for bit; spread bit for bit except a NaN of the arithmetic's own making."""
    assert grecs.shape == erecs.shape, (tag, what)
    exact = [0, 2, 3, 4]
    bad = np.argwhere(grecs[:, :, exact] != erecs[:, :, exact])
    assert bad.size == 0, (tag, what, "pace / counts", bad[:8].tolist(), grecs[tuple(bad[0][:2])], erecs[tuple(bad[0][:2])])
    gs, es = grecs[:, :, 1], erecs[:, :, 1]
    made = np.isnan(es.view(np.float32)) & (erecs[:, :, 0] != NAN_BITS)
    assert np.array_equal(np.isnan(gs.view(np.float32)), np.isnan(es.view(np.float32))), (tag, what, "spread NaN masks")
    bad = np.argwhere((gs != es) & ~made)
    assert bad.size == 0, (tag, what, "spread", bad[:8].tolist(), gs[tuple(bad.T)][:8], es[tuple(bad.T)][:8])


def _compare_sums(grecs, erecs, terms, tag):
    """part 1 is +0.0; part 0 within the tolerance of a sum taken in another order"""
    assert (grecs[:, 1, 5:] == 0).all(), (tag, "section sums")
    g, e = grecs[:, 0, 5:].view(np.float32).astype(np.float64), erecs[:, 0, 5:].view(np.float32).astype(np.float64)
    fin = np.isfinite(e)
    assert np.array_equal(np.isnan(g), np.isnan(e)) and np.array_equal(np.isposinf(g), np.isposinf(e)) and \
        np.array_equal(np.isneginf(g), np.isneginf(e)), (tag, "non-finite sums", g[~fin], e[~fin])
    if fin.any():
        err = np.abs(g[fin] - e[fin]) / np.maximum(1.0, terms[fin])
        print(tag, "sums: max error", float(err.max()), "of", int(fin.sum()))
        assert err.max() <= 2e-6, (tag, "sums", float(err.max()))


def _compare(got, exp, tag):
    (gpairs, gcols, gnodes, granks), (epairs, ecols, enodes, eranks, terms) = got, exp
    _compare_exact(gpairs, epairs, tag, "A")
    _compare_exact(gcols, ecols, tag, "B")
    _compare_records(gnodes, enodes, tag, "C")
    assert (gnodes[:, :, 5:] == 0).all(), (tag, "C's sum slots")
    _compare_records(granks, eranks, tag, "D")
    _compare_sums(granks, eranks, terms, tag)


@pytest.mark.parametrize("R,K,S,layout", node_cases.CASES)
def test_node_score_matches_numpy(be, R, K, S, layout):
    from nvrx_straggler.backend import PeerGroups

    labels = node_cases.labels_of(R, layout)
    nodes = PeerGroups(labels)
    G, largest = nodes.G, nodes.max_size
    results = []
    for t, T in enumerate(node_cases.tables(R, K, S, labels)):
        for min_members, min_nodes in node_cases.THRESHOLDS:
            tag = (R, K, S, layout, t, min_members, min_nodes)
            got = _run(be, T, K, S, nodes, min_members, min_nodes, 0, R)
            exp = node_scores_table(T, K, S, nodes.host, G, largest, min_members, min_nodes, 0, R)
            _compare(got, exp, tag)
            results.append(exp)
        # a window of ranks that starts and ends inside a node equals the slice of the full result, bit for bit
        lo, n = (R // 3, max(1, R // 2)) if R > 1 else (0, 1)
        part = _run(be, T, K, S, nodes, 1, 1, lo, n)
        for x, y, what in zip(part[:3], got[:3], "ABC"):
            assert np.array_equal(x, y), (R, K, S, layout, t, "window", what)
        assert np.array_equal(part[3], got[3][lo : lo + n]), (R, K, S, layout, t, "window", "D")
    node_cases.check_properties(node_cases.case_properties(results, G), labels)


@pytest.mark.parametrize("R,K,S,layout", [(8, 65, 2, "mod:2"), (64, 17, 33, "block:8"), (65, 70, 5, "block:5"),
                                          (100, 7, 9, "65+35"), (1025, 3, 2, "mod:17")])
def test_block_a_is_the_column_block_of_the_pace_scores_per_peer_group(be, R, K, S, layout):
    from nvrx_straggler.backend import PeerGroups

    nodes = PeerGroups(node_cases.labels_of(R, layout))
    for t, T in enumerate(node_cases.tables(R, K, S, nodes.group.tolist())):
        for min_members in (2, 1):
            pairs = _run(be, T, K, S, nodes, min_members, 3, 0, R)[0]
            ws = be.workspace(R, K, S, R, 0)
            cols, _ = be.pace_group_score(ws, ws.send, nodes, 0, R, min_members, 1).records()
            _compare_exact(pairs, cols, (R, K, S, layout, t, min_members), "A")


@pytest.mark.parametrize("R,K,S", [(8, 65, 2), (64, 17, 33), (65, 70, 5), (3, 4097, 0), (130, 3, 2)])
def test_every_rank_its_own_node_is_the_job_wide_pace_score(be, R, K, S):
    """With single-member nodes and ``min_members = 1`` a node's med is its rank's value: B and D are ``nvrx_pace_score``'s
    columns and rank records (``min_ranks = min_nodes``), and C is D without the sums.  Exact words bit for bit; the sums (two
    launches of the rank kernel need not add in one order) get the bound above."""
    from nvrx_straggler.backend import PeerGroups

    nodes = PeerGroups(list(range(R)))
    for t, T in enumerate(node_cases.tables(R, K, S, list(range(R)))):
        for min_nodes in (1, min(3, R)):
            tag = (R, K, S, t, min_nodes)
            pairs, bcols, nrecs, rrecs = _run(be, T, K, S, nodes, 1, min_nodes, 0, R)
            ws = be.workspace(R, K, S, R, 0)
            cols, recs = be.pace_score(ws, ws.send, 0, R, min_nodes).records()
            terms = pace_scores_table(T, K, S, 0, R, min_nodes)[2]
            _compare_exact(bcols, cols, tag, "B")
            _compare_records(rrecs, recs, tag, "D")
            _compare_sums(rrecs, recs, terms, tag)
            _compare_records(nrecs, rrecs, tag, "C against D")
            assert (nrecs[:, :, 5:] == 0).all(), (tag, "C's sum slots")


def test_out_of_range_node_contents_are_guarded(be):
    """Node ids outside [0, G), members outside [0, R), ``start`` words negative, decreasing and beyond R, stretches that
    overlap (the one content that takes the fused kernel off its every-node-at-once path) and a stretch above ``max_group``:
    the result is what the restatement says, and no word outside NVRX_NODE_WORDS of a guard-padded buffer is
    touched.  Valid launches only: the kernels' guards keep every access inside the table, the array and the buffer -- and the
    table has spare rows behind R, so that even a member index the guards let through would land in memory the test owns."""
    from nvrx_straggler import _native
    from nvrx_straggler.backend import PeerGroups

    PAD, FILL, SPARE = 64, 0x5A5A5A5A, 16
    rng = np.random.default_rng(83)
    # the fused kernel (nodes of 5 or 6, once cut to 4), and the two-launch path (nodes of 66 and 4, cut to 65)
    for R, K, S, labels, largest in ((21, 5, 70, [r % 4 for r in range(21)], 6), (21, 5, 70, [r % 4 for r in range(21)], 4),
                                     (70, 66, 3, [1 if r % 17 == 3 else 0 for r in range(70)], 65)):
        G = max(labels) + 1
        T = random_table(rng, R + SPARE, K, S)
        good = PeerGroups(labels).host
        cases = {"intact": good.copy()}
        a = cases["node id G and -1"] = good.copy()
        a[3], a[8] = G, -1
        a = cases["member R and -1"] = good.copy()
        a[R + 2], a[R + 9] = R, -1
        a = cases["start beyond R"] = good.copy()
        a[2 * R + G] = R + 5
        a = cases["start below 0 and descending"] = good.copy()
        a[2 * R], a[2 * R + 1] = -3, 0
        if G > 2:
            a[2 * R + 2] = 1
        if G > 2:  # node 0 takes members 0 .. 7, node 1 none, node 2 members 4 .. again: the fused kernel's loop over the nodes
            a = cases["stretches that overlap"] = good.copy()
            a[2 * R + 1], a[2 * R + 2] = 8, 4
        a = cases["everything"] = good.copy()
        a[0], a[R + R - 1], a[2 * R + G], a[2 * R + 1] = G + 7, 1 << 30, 1 << 30, -(1 << 30)
        table = torch.from_numpy(T).cuda()
        for name, arrays in cases.items():
            for first, n in ((0, R), (4, 9)):
                words = _native.node_words(G, n, K, S)
                out = torch.full((PAD + words + PAD,), FILL, dtype=torch.int32, device="cuda")
                d_nodes = torch.from_numpy(arrays).cuda()
                torch.cuda.synchronize()
                rc = be.lib.nvrx_node_score(table.data_ptr(), R, K, S, d_nodes.data_ptr(), G, largest, 2, 3, first, n,
                                            out.data_ptr() + 4 * PAD, be._stream_handle)
                assert rc == 0, (name, be.lib.nvrx_last_error())
                be.synchronize()
                torch.cuda.synchronize()
                host = out.cpu().numpy().view(np.uint32)
                assert (host[:PAD] == FILL).all() and (host[PAD + words :] == FILL).all(), (R, name)
                body = host[PAD : PAD + words]
                KS = K + S
                a_, b_, c_ = 4 * G * KS, 4 * G * KS + 4 * KS, 4 * G * KS + 4 * KS + 16 * G
                got = (body[:a_].reshape(G, KS, 4), body[a_:b_].reshape(KS, 4), body[b_:c_].reshape(G, 2, 8),
                       body[c_:].reshape(n, 2, 8))
                _compare(got, node_scores_table(T[:R], K, S, arrays, G, largest, 2, 3, first, n), (R, largest, name, first, n))
                if name == "intact":
                    assert int(got[0][0, :, 1].max()) <= largest  # a stretch above max_group is cut


def test_argument_errors_come_back_before_the_device_is_touched(be):
    import ctypes

    from nvrx_straggler import _native
    from nvrx_straggler.backend import PeerGroups

    lib = be.lib
    R, K, S, G = 8, 8, 2, 2
    table = torch.zeros((R, _native.table_len(K, S)), dtype=torch.float32, device="cuda")
    out = torch.full((_native.node_words(G, R, K, S),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    d_nodes = torch.from_numpy(PeerGroups([r % G for r in range(R)]).host).cuda()
    torch.cuda.synchronize()

    def score(tp=table.data_ptr(), R=R, gp=d_nodes.data_ptr(), G=G, largest=4, min_members=2, min_nodes=3, first=0, n=R,
              op=out.data_ptr()):
        return lib.nvrx_node_score(tp, R, K, S, gp, G, largest, min_members, min_nodes, first, n, op, be._stream_handle)

    def said(text):
        return text in lib.nvrx_last_error().decode()

    assert score(tp=None) == _native.ERR_INVALID and score(gp=None) == _native.ERR_INVALID and score(op=None) == _native.ERR_INVALID
    assert score(R=_native.ROBUST_MAX_RANKS + 1, n=1) == _native.ERR_RANGE
    assert score(first=7, n=2) == _native.ERR_RANGE and score(first=-1) == _native.ERR_RANGE and score(n=R + 1) == _native.ERR_RANGE
    assert score(G=0) == _native.ERR_INVALID and score(G=R + 1) == _native.ERR_RANGE
    assert score(largest=0) == _native.ERR_RANGE and score(largest=R + 1) == _native.ERR_RANGE
    assert score(min_members=0) == _native.ERR_RANGE and score(min_nodes=0) == _native.ERR_RANGE
    assert score(op=out.data_ptr() + 4) == _native.ERR_INVALID
    # the stated order: the shape and the ranks, then G, then max_group, then the two thresholds, then the pointers
    assert score(R=0, first=5, n=4, G=0, largest=0, min_members=0, min_nodes=0, tp=None) == _native.ERR_INVALID and said("shape")
    assert score(first=5, n=4, G=0, largest=0, min_members=0, min_nodes=0, tp=None) == _native.ERR_RANGE and said("outside")
    assert score(G=0, largest=0, min_members=0, min_nodes=0, tp=None) == _native.ERR_INVALID and said("groups")
    assert score(G=R + 1, largest=0, min_members=0, min_nodes=0, tp=None) == _native.ERR_RANGE and said("groups")
    assert score(largest=0, min_members=0, min_nodes=0, tp=None) == _native.ERR_RANGE and said("max_group")
    assert score(min_members=0, min_nodes=0, tp=None) == _native.ERR_RANGE and said("min_members")
    assert score(min_nodes=0, tp=None) == _native.ERR_RANGE and said("min_nodes")
    desc = _native.ReportDesc()
    desc.R, desc.K, desc.S = R, K, S
    gp = d_nodes.data_ptr()
    assert lib.nvrx_report_node(None, ctypes.byref(desc), gp, G, 4, 2, 3, 0, R, out.data_ptr()) == _native.ERR_INVALID
    rings = be.make_rings(1, 4, 16)
    try:  # a context no report went through this descriptor on
        assert lib.nvrx_report_node(rings.ctx, ctypes.byref(desc), gp, G, 9, 2, 3, 0, R, out.data_ptr()) == _native.ERR_RANGE
        assert lib.nvrx_report_node(rings.ctx, ctypes.byref(desc), None, G, 4, 2, 3, 0, R, out.data_ptr()) == _native.ERR_INVALID
        assert lib.nvrx_report_node(rings.ctx, ctypes.byref(desc), gp, G, 4, 2, 3, 0, R, out.data_ptr()) == _native.ERR_STATE
    finally:
        rings.close()
    be.synchronize()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x5A5A5A5A).all()  # nothing was launched


# ---- the node step of a report ------------------------------------------------------------------------------------------------
def _same_as_direct(rep, tag, min_members, min_nodes):
    """What the report's node step wrote IS what ``nvrx_node_score`` says of the same table (same kernels, same order of sums:
    every word equal), and both are what the restatement says of it."""
    R, K, S = rep["shape"]
    t = rep["node"]
    pairs, cols, nrecs, rrecs = rep["direct"]
    host, G, largest = rep["nodes"]
    _compare(rep["direct"], node_scores_table(rep["table"], K, S, host, G, largest, min_members, min_nodes, 0, R), tag)
    assert t["params"]["min_members"] == min_members and t["params"]["min_nodes"] == min_nodes
    labels = list(t["nodes"])
    for recs, shown, keys in ((rrecs, t["ranks"], range(R)), (nrecs, t["node_scores"], labels)):
        f = recs.view(np.float32)
        for i, key in enumerate(keys):
            for p, part in enumerate(("gpu", "sections")):
                d = shown[key][part]
                assert [d["columns"], d["slower"], d["faster"]] == recs[i, p, 2:5].tolist(), (tag, key, part)
                assert (d["pace"] == float(f[i, p, 0]) or recs[i, p, 0] == NAN_BITS) and \
                    (d["spread"] == float(f[i, p, 1]) or np.isnan(f[i, p, 1])), (tag, key, part)
    f = rrecs.view(np.float32)
    for r in range(R):
        gpu = t["ranks"][r]["gpu"]
        assert [gpu["total_us"], gpu["slower_us"], gpu["excess_us"]] == f[r, 0, 5:].tolist(), (tag, r)
    columns = list(t["kernels"].values()) + list(t["section_columns"].values())
    shown = sorted((x["center"], x["nodes"], x["above"], x["below"]) for x in columns)
    want = sorted((float(c), int(n), int(a), int(b)) for c, (n, a, b) in zip(cols[:, 0].copy().view(np.float32), cols[:, 1:]))
    assert repr(shown) == repr(want), tag  # (repr: a NaN centre equals a NaN centre)
    per_node = sorted((labels.index(g), x["median"], x["ranks"]) for c in columns for g, x in c["per_node"].items())
    want = sorted((g, float(m), int(n)) for g in range(G) for m, n in zip(pairs[g, :, 0].copy().view(np.float32), pairs[g, :, 1]))
    assert repr(per_node) == repr(want), tag


def _check_reports(reports, fused_want):
    assert [r["fused"] for r in reports] == fused_want
    compared = 0
    for i, rep in enumerate(reports):
        assert rep["nodes_named"] == [workers.SLOW_NODE] and rep["alone"] == [workers.SLOW_RANK], (i, rep["nodes_named"], rep["alone"])
        assert rep["pace_named"] == [workers.SLOW_RANK] + workers.SLOW_NODE_RANKS, (i, rep["pace_named"])
        t = rep["node"]
        assert sorted(t["ranks"]) == list(range(workers.RANKS)) and sorted(t["kernels"]) == sorted(workers.KERNEL_NAMES)
        assert t["nodes"] == {g: list(range(8 * g, 8 * g + 8)) for g in range(4)} and t["unrated_nodes"] == []
        slow = t["node_scores"][workers.SLOW_NODE]
        assert slow["gpu"]["slower"] == 120 and slow["gpu"]["columns"] == 120 and slow["members_off_pace"] == 8
        assert all(t["node_scores"][g]["gpu"]["breadth"] < 0.9 for g in range(4) if g != workers.SLOW_NODE)
        if "direct" not in rep:
            continue
        compared += 1
        assert rep["shape"] == (workers.RANKS, 120, 1)
        _same_as_direct(rep, ("report", i), 2, 3)
    assert compared >= 2


@pytest.mark.parametrize("asynchronous", [False, True])
def test_report_step_on_the_general_and_the_one_call_path(be, asynchronous):
    _check_reports(workers.folded_node(0, 1, asynchronous=asynchronous), [False, True, True])


def test_report_step_behind_a_report_that_was_scored_resident():
    """``nvrx_report_node``'s ordering: the score kernel ran on a stream of its own, the node kernels follow it by an event."""
    res = run_ranks(workers.folded_node_sync_then_async, 1, timeout=300, use_oracle_backend=False, device=0,
                    env={"NVRX_DEBUG_RESIDENT_SCORER": "2"})[0]
    for mode in ("sync", "async"):
        _check_reports(res[mode], [False, True, True])


def test_report_step_behind_reports_that_were_rehomed():
    """Asynchronous Detector reports re-homed onto the stream of their stamps: every report's node step read its own window,
    and wrote what ``nvrx_node_score`` says of that window's table."""
    res = run_ranks(workers.detector_rehomed, 1, timeout=300, use_oracle_backend=False, device=0,
                    env={"NVRX_DEBUG_ASYNC_REHOME_GAP_US": "1"})[0]
    assert res["rehomed"] > 0 and res["lane_is_none"]
    compared = 0
    for t, rep in enumerate(res["reports"], start=1):
        scores = rep["node"]
        for i in range(3):
            assert scores["section_columns"][f"s{i}"] == {"center": float(10 * t + i), "nodes": 1, "above": 0, "below": 0,
                                                          "per_node": {"n": {"median": float(10 * t + i), "ranks": 1}}}, (t, i)
        want = {"pace": 1.0, "spread": 0.0, "columns": 3, "slower": 0, "faster": 0, "breadth": 0.0}
        assert scores["ranks"][0]["sections"] == want
        assert {k: scores["node_scores"]["n"]["sections"][k] for k in want} == want
        assert scores["ranks"][0]["gpu"]["pace"] == 1.0 and scores["ranks"][0]["gpu"]["columns"] == 3
        assert scores["unrated_nodes"] == []
        if "direct" in rep:
            compared += 1
            assert rep["shape"][0] == 1 and rep["shape"][1] >= 3 and rep["shape"][2] >= 3, rep["shape"]
            _same_as_direct(rep, ("re-homed", t), 1, 1)
    assert compared >= len(res["reports"]) - 1


@pytest.mark.parametrize("asynchronous", [False, True])
def test_option_off_leaves_the_real_workspace_without_a_node_buffer(asynchronous):
    """With the option off nothing is allocated, resolved or launched: after a general and three planned reports the
    workspace the reports ran on has no node buffer and no node step in flight, and no workspace of the backend gained one."""
    res = workers.folded_option_off(0, 1, asynchronous=asynchronous)
    assert res["option"] is False and res["resolved"] is None
    assert res["said"] == [({}, True, False)] * 4 and res["fused"] == [False, True, True, True], (res["said"], res["fused"])
    assert res["planned_ws"] == (None, None, False, (6, 2, 1)), res["planned_ws"]
    assert res["new"] == []


def test_a_report_held_across_the_next_two_is_still_its_own():
    out = workers.held_reports(0, 1)
    assert len(out) == 5
    for w, t in enumerate(out):
        # mod:2 -- node 0 = ranks {0, 2} at 10 (w + 1) + {0, 2}, node 1 = ranks {1, 3} at + {1, 3}: lower medians base and
        # base + 1, and the nodes' centre their lower median, base
        base = 10.0 * (w + 1)
        assert t["kernels"]["gemm"] == {"center": base, "nodes": 2, "above": 1, "below": 0,
                                        "per_node": {0: {"median": base, "ranks": 2}, 1: {"median": base + 1.0, "ranks": 2}}}, (w, t["kernels"])
        assert t["section_columns"]["step"]["center"] == 100.0 * (w + 1)
        assert t["node_scores"][1]["gpu"]["pace"] == float(np.float32(base / (base + 1.0)))
        assert t["ranks"][3]["gpu"]["pace"] == float(np.float32(base / (base + 3.0)))
        assert t["node_scores"][0]["gpu"]["pace"] == 1.0 and t["node_of"] == {0: 0, 1: 1, 2: 0, 3: 1}


def test_the_example_names_node_2_alone_where_the_pace_rule_names_nine_ranks():
    out = subprocess.run([sys.executable, os.path.join(REPO, "examples", "straggler_example.py"), "--node"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert re.findall(r"identify_pace_stragglers\(\): (\[[^\]]*\])", out.stdout) == ["[5, 16, 17, 18, 19, 20, 21, 22, 23]"], out.stdout
    assert re.findall(r"identify_node_stragglers\(\) nodes: (\[[^\]]*\])", out.stdout) == ["[2]"], out.stdout
    assert re.findall(r"identify_node_stragglers\(\) ranks off pace alone: (\[[^\]]*\])", out.stdout) == ["[5]"], out.stdout
    assert re.search(r"node 2 \(ranks 16-23\): pace 0\.96\d+ .* in 120 / 0 of 120 kernels, 8 of 8 ranks off pace", out.stdout), out.stdout
