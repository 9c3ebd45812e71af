"""Node scores per peer group on the GPU: ``nvrx_node_group_score`` on a guard-padded ``d_out`` against the plain NumPy restatement
below (sort and index, f64 quotients), and the report step.  A, B, C and the exact words of D bit for bit (a NaN the arithmetic
itself makes by NaN-ness only); D's three sums as tests/test_gpu_node.py compares them (``_compare_sums``: 2e-6 * max(1, sum of
|terms|), an f64 weighted sum taken in another order)."""
import numpy as np
import pytest
import torch

from score_cases import random_table
from test_gpu_node import _compare_exact, _compare_records, _compare_sums

pytestmark = pytest.mark.gpu

NAN = 0x7FC00000
PAD, FILL = 64, 0x5A5A5A5A


@pytest.fixture(scope="module")
def be():
    from nvrx_straggler.backend import get_backend

    return get_backend()


def _key(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u >> 31, ~u, u | np.uint32(0x80000000))


def _median_record(values, need):
    """{lower median by key (NaN below ``need``), n, above, below} of f32 ``values``, all of them counted."""
    n = values.size
    if n == 0:
        return [NAN, 0, 0, 0]
    order = np.argsort(_key(values), kind="stable")
    m = values[order[(n - 1) >> 1]]
    return [int(m.view(np.uint32)) if n >= need else NAN, n, int((_key(values) > _key(m)).sum()), int((_key(values) < _key(m)).sum())]


def _pace_record(v, ctr, w):
    """nvrx_pace_score's record of values ``v`` against centres ``ctr`` (NaN: not referenced); ``w``: the weights, or None."""
    rec, terms = np.zeros(8, dtype=np.uint32), np.zeros(3)
    with np.errstate(all="ignore"):
        eligible = (v >= 0) & ~np.isnan(ctr)
        quot = ctr.astype(np.float64) / v.astype(np.float64)
        q = quot.astype(np.float32)
        has_q = eligible & ~np.isnan(q)
        slower, faster = eligible & (_key(v) > _key(ctr)), eligible & (_key(v) < _key(ctr))
        rec[0] = rec[1] = NAN
        rec[2:5] = eligible.sum(), slower.sum(), faster.sum()
        if has_q.any():
            qs = q[has_q]
            pace = qs[np.argsort(_key(qs), kind="stable")[(qs.size - 1) >> 1]]
            dev = np.sort((qs - pace).astype(np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF))
            rec[0], rec[1] = pace.view(np.uint32), dev[(qs.size - 1) >> 1]
        if w is not None:
            w = w.astype(np.float64)
            ex = w[has_q] * (1.0 - quot[has_q])
            rec[5:8] = np.array([w[eligible].sum(), w[slower].sum(), ex.sum()], dtype=np.float32).view(np.uint32)
            terms[:] = np.abs(w[eligible]).sum(), np.abs(w[slower]).sum(), np.abs(ex).sum()
    return rec, terms


def restate(T, K, S, cells, min_members, min_nodes, min_peers, first, n):
    """(A, B, C, D, terms of D's sums) for the VALID cell array of ``cells`` (a backend.NodeCells)."""
    KS = K + S
    (C, Gp, Gn), R = cells.G, cells.R
    cell_of, cgroup, rgroup = cells.host[:R], cells.cell_group, cells.peers.group
    A, B = np.zeros((C, KS, 4), dtype=np.uint32), np.zeros((Gp, KS, 4), dtype=np.uint32)
    for j in range(C):
        rows = T[cell_of == j, :KS]
        for c in range(KS):
            A[j, c] = _median_record(rows[rows[:, c] >= 0, c], max(1, min(min_members, rows.shape[0])))
    med = A[:, :, 0].copy().view(np.float32)
    for p in range(Gp):
        mine = med[cgroup == p]
        for c in range(KS):
            B[p, c] = _median_record(mine[~np.isnan(mine[:, c]), c], max(min_peers, min(min_nodes, mine.shape[0])))
    ctr = B[:, :, 0].copy().view(np.float32)
    Cb, D, terms = np.zeros((Gn, 2, 8), dtype=np.uint32), np.zeros((n, 2, 8), dtype=np.uint32), np.zeros((n, 3))
    for p, (lo, hi) in enumerate(((0, K), (K, KS))):
        for g in range(Gn):
            own = cells.cells_of_node(g)
            Cb[g, p] = _pace_record(med[own, lo:hi].ravel(), ctr[cgroup[own], lo:hi].ravel(), None)[0]
        for i in range(n):
            r = first + i
            D[i, p], t = _pace_record(T[r, lo:hi], ctr[rgroup[r], lo:hi], T[r, 2 * KS : 2 * KS + K] if p == 0 else None)
            if p == 0:
                terms[i] = t
    return A, B, Cb, D, terms


def _table(seed, R, K, S, spare=0):
    """random_table with absent values, and every other column quantised to steps of 0.5: ties and duplicates."""
    T = random_table(np.random.default_rng(seed), R + spare, K, S)
    med = T[:, : K + S : 2]
    T[:, : K + S : 2] = np.where(med >= 0, np.maximum(np.round(med * 2) / 2, 0.5), med)
    return T


def _cells(node_of, group_of):
    from nvrx_straggler.backend import NodeCells, PeerGroups

    return NodeCells(PeerGroups(list(node_of)), PeerGroups(list(group_of)))


def _run(be, d_table, R, K, S, cells, array, thresholds, first, n):
    """nvrx_node_group_score on a guard-padded buffer -> (A, B, C, D); the canaries are checked."""
    from nvrx_straggler import _native

    words = _native.node_group_words(*cells.G, n, K, S)
    out = torch.full((PAD + words + PAD,), FILL, dtype=torch.int32, device="cuda")
    d_cells = torch.from_numpy(array).cuda()
    torch.cuda.synchronize()
    rc = be.lib.nvrx_node_group_score(d_table.data_ptr(), R, K, S, d_cells.data_ptr(), *cells.G, *cells.maxima, *thresholds, first, n,
                                      out.data_ptr() + 4 * PAD, be._stream_handle)
    assert rc == 0, be.lib.nvrx_last_error()
    be.synchronize()
    torch.cuda.synchronize()
    host = out.cpu().numpy().view(np.uint32)
    assert (host[:PAD] == FILL).all() and (host[PAD + words :] == FILL).all(), "canaries"
    C, Gp, Gn = cells.G
    KS, body = K + S, host[PAD : PAD + words]
    a, b, c = 4 * C * KS, 4 * (C + Gp) * KS, 4 * (C + Gp) * KS + 16 * Gn
    return body[:a].reshape(C, KS, 4), body[a:b].reshape(Gp, KS, 4), body[b:c].reshape(Gn, 2, 8), body[c:].reshape(n, 2, 8)


def _loaded(be, T, K, S):
    ws = be.workspace(T.shape[0], K, S, T.shape[0], 0)
    ws.node_settle(), ws.pace_settle()
    ws.send.copy_(torch.from_numpy(T))
    torch.cuda.synchronize()
    return ws


def _compare(got, exp, tag):
    for x, y, what in zip(got[:2], exp[:2], "AB"):
        _compare_exact(x, y, tag, what)
    _compare_records(got[2], exp[2], tag, "C")
    assert (got[2][:, :, 5:] == 0).all(), (tag, "C's sum slots")
    _compare_records(got[3], exp[3], tag, "D")
    _compare_sums(got[3], exp[3], exp[4], tag)


ALL = ((2, 3, 2), (1, 1, 1), (200, 200, 2))  # (min_members, min_nodes, min_peers): the defaults, none, above every size
SPLIT = ([0, 0, 1, 1, 2, 2, 2, 3].__getitem__, [0, 0, 1, 1, 1, 2, 2, 2].__getitem__)  # (node, group) of 8 ranks, see below
# (R, K, S, node of rank r, peer group of rank r, thresholds, (first_rank, n_ranks) or None) -- what each is there for:
CASES = {
    "2 groups x 2 nodes, K+S = 1": (8, 1, 0, lambda r: r // 2, lambda r: r // 4, ALL, None),
    # group 0 sits on node 0 alone (unreferenced in B at min_peers = 2, node 0 unrated), node 2 spans groups 1 and 2; K+S = 65;
    # 2 cells x 60 columns: the register form of the node kernel
    "a node in two groups, a group on one node": (8, 60, 5, *SPLIT, ALL, (3, 4)),
    "2 cells x 2100 columns: the re-reading node kernel": (8, 2100, 1, *SPLIT, ((2, 3, 2),), None),
    "R = 64, C = 64, K+S = 64, groups of 22, 21, 21": (64, 40, 24, lambda r: r, lambda r: r % 3, ALL, None),
    "R = 65: the first shape in two launches": (65, 3, 2, lambda r: r // 5, lambda r: r % 2, ALL, (7, 50)),
    "groups of 64 and 33 cells: the wave form at its edge": (130, 2, 3, lambda r: r if r < 64 else 64 + (r - 64) // 2,
                                                            lambda r: int(r >= 64), ALL, None),
    "groups of 64, 65 and 1 cells: the radix form": (131, 3, 1, lambda r: r, lambda r: 0 if r < 64 else 1 if r < 129 else 2,
                                                    ((2, 3, 2), (1, 1, 1)), None),
    "a cell of 70 ranks": (100, 2, 2, lambda r: 0 if r < 70 else 1 + (r - 70) // 10, lambda r: int(r >= 85), ALL, (60, 40)),
}


@pytest.mark.parametrize("case", CASES)
def test_matches_the_numpy_restatement(be, case):
    R, K, S, node_of, group_of, thresholds, window = CASES[case]
    cells = _cells(map(node_of, range(R)), map(group_of, range(R)))
    T = _table(len(case), R, K, S)
    d_table = torch.from_numpy(T).cuda()
    for thr in thresholds:
        for first, n in ((0, R),) + ((window,) if window else ()):
            got = _run(be, d_table, R, K, S, cells, cells.host, thr, first, n)
            _compare(got, restate(T, K, S, cells, *thr, first, n), (case, thr, first, n))
    if case.startswith("a node in two groups"):
        assert np.isnan(got[1][0, :, 0].view(np.float32)).all() and (got[2][0, :, 2] == 0).all()  # group 0 and node 0 (thr[2] = 2)
        assert (got[2][2, 0, 2] > K).any()  # node 2 counts pairs: more columns than kernels


@pytest.mark.parametrize("R,K,S,layout", [(40, 9, 3, "mod:5"), (100, 5, 66, "block:10")])
def test_one_peer_group_is_the_job_wide_node_score(be, R, K, S, layout):
    from nvrx_straggler.backend import PeerGroups

    kind, step = layout.split(":")
    node_of = [r % int(step) if kind == "mod" else r // int(step) for r in range(R)]
    cells, nodes = _cells(node_of, [0] * R), PeerGroups(node_of)
    T = _table(R, R, K, S)
    ws = _loaded(be, T, K, S)
    for min_members, min_nodes in ((2, 3), (1, 1)):
        pairs, cols, nrecs, rrecs = be.node_score(ws, ws.send, nodes, 0, R, min_members, min_nodes).records()
        got = _run(be, ws.send, R, K, S, cells, cells.host, (min_members, min_nodes, 1), 0, R)
        tag = (R, layout, min_members, min_nodes)
        for x, y, what in ((got[0], pairs, "A"), (got[1][0], cols, "B"), (got[2], nrecs, "C")):
            _compare_exact(x, y, tag, what)
        _compare_records(got[3], rrecs, tag, "D")
        _compare_sums(got[3], rrecs, restate(T, K, S, cells, min_members, min_nodes, 1, 0, R)[4], tag)


@pytest.mark.parametrize("R,K,S,step", [(12, 5, 2, 3), (70, 3, 66, 2)])
def test_every_rank_its_own_node_is_the_pace_score_per_peer_group(be, R, K, S, step):
    from nvrx_straggler.backend import PeerGroups

    group_of = [r % step for r in range(R)]
    cells, groups = _cells(range(R), group_of), PeerGroups(group_of)
    T = _table(R, R, K, S)
    ws = _loaded(be, T, K, S)
    for min_nodes, min_peers in ((3, 2), (1, 1), (200, 2)):
        cols, recs = be.pace_group_score(ws, ws.send, groups, 0, R, min_nodes, min_peers).records()
        got = _run(be, ws.send, R, K, S, cells, cells.host, (1, min_nodes, min_peers), 0, R)
        tag = (R, step, min_nodes, min_peers)
        _compare_exact(got[1], cols, tag, "B")
        _compare_records(got[3], recs, tag, "D")
        _compare_sums(got[3], recs, restate(T, K, S, cells, 1, min_nodes, min_peers, 0, R)[4], tag)


@pytest.mark.parametrize("R", [12, 70])
def test_a_damaged_array_stays_inside_and_leaves_the_other_cells_alone(be, R):
    """The canaries hold (``_run``) and every record the damage has no part in is what it was; the table has spare rows behind R."""
    K, S = 4, 63
    cells = _cells([r // 3 for r in range(R)], [r // (R // 3) for r in range(R)])  # a group's ranks lie on some of the nodes
    (C, Gp, Gn), thr = cells.G, (2, 3, 2)
    d_table = torch.from_numpy(_table(R, R, K, S, spare=16)).cuda()
    intact = _run(be, d_table, R, K, S, cells, cells.host, thr, 0, R)
    bad = cells.host.copy()
    cell, node = 1, Gn - 1                         # the cell that loses a member, the node whose list names a cell C
    bad[R + int(bad[2 * R + cell])] = R            # members[cstart[cell]]
    bad[2 * R + C] = R + 5                         # cstart[C]: clamped to R, which is its value
    nstart = bad[2 * R + C + 1 + Gp + 1 :]
    bad[2 * R + C + 1 + Gp + 1 + Gn + 1 + int(nstart[node])] = C  # the first entry of that node's list
    got = _run(be, d_table, R, K, S, cells, bad, thr, 0, R)
    group = int(cells.cell_group[cell])
    nodes_ok = np.array([g != node and group not in cells.cell_group[cells.cells_of_node(g)] for g in range(Gn)])
    for x, y, keep in zip(got, intact, (np.arange(C) != cell, np.arange(Gp) != group, nodes_ok, cells.peers.group != group)):
        assert keep.any() and np.array_equal(x[keep], y[keep])
    assert not np.array_equal(got[0][cell], intact[0][cell])  # (the damage was seen at all)


RANKS, PER_NODE, KERNELS, SAMPLES = 64, 8, 120, 50


def _job_medians():  # the job of examples/straggler_example.py --node-peer
    rng = np.random.default_rng(2026)
    base = rng.lognormal(np.log(1000.0 / KERNELS), 0.5, KERNELS)
    med = base[None, :] * (1.0 + 0.01 * rng.standard_normal((RANKS, KERNELS)))
    med[RANKS // 2 :] *= 1.5
    med[5 * PER_NODE : 6 * PER_NODE] *= 1.04
    med[3] *= 1.04
    return med.astype(np.float32)


def _reports(be, asynchronous, node_peer_groups, reports=2):
    from nvrx_straggler.folded import FoldedJob

    med = _job_medians()
    job = FoldedJob(total_ranks=RANKS, section_names=["step"], ring_cap=64, scores_to_compute=("relative_perf_scores",),
                    kernel_names=[f"kernel_{k:03d}" for k in range(KERNELS)], node_scores=True, node_groups=f"block:{PER_NODE}",
                    peer_groups="block:32", asynchronous=asynchronous, node_peer_groups=node_peer_groups)
    try:
        out = []
        for _ in range(reports):
            for lr, r in enumerate(job.logical_ranks()):
                job.load(lr, np.full((1, SAMPLES), med[r].sum(), dtype=np.float32))
                job.load_kernels(lr, np.repeat(med[r][:, None], SAMPLES, axis=1))
            rep = job.report()
            found = rep.identify_node_stragglers()
            entry = {"scores": rep.node_scores(), "nodes": sorted(found["straggler_nodes"]),
                     "alone": sorted(s.rank for s in found["ranks_off_pace_alone"])}
            out.append(entry)
            rpt = job.reporter
            if rpt._ring_plan is not None:  # (the first report takes the general path and plans the next ones)
                ws = rpt._ring_plan.ws
                be.synchronize()
                entry["family"] = ws._table_state["node"].last.family.name
                if node_peer_groups:
                    cells = rpt._cells_for(rpt._node_for(ws), rpt._peer_for(ws))
                    entry["direct"] = _run(be, ws.table, ws.R, ws.K, ws.S, cells, cells.host, (2, 3, 2), 0, ws.R)
        return out
    finally:
        job.close()


@pytest.mark.parametrize("asynchronous", [False, True])
def test_report_step_on_says_what_the_direct_call_says_and_off_what_it_said(be, asynchronous):
    for rep in _reports(be, asynchronous, False):  # off: the job-wide step, the lockstep rule on a pipeline job, the old dict
        t = rep["scores"]
        assert rep.get("family", "node") == "node" and rep["nodes"] == [4, 5, 6, 7]
        assert not {"peer_groups", "groups", "group_of", "cells", "per_node"} & set(t)
        assert set(t["kernels"]["kernel_000"]) == {"center", "nodes", "above", "below", "per_node"}
    reports = _reports(be, asynchronous, True)
    assert "direct" in reports[-1]
    for rep in reports:
        assert (rep["nodes"], rep["alone"]) == ([5], [3])
        if "direct" not in rep:
            continue
        t, (A, B, Cb, D) = rep["scores"], rep["direct"]
        assert rep["family"] == "node_group" and t["peer_groups"] is True and t["params"]["min_peers"] == 2
        assert t["groups"] == {0: list(range(32)), 1: list(range(32, 64))} and t["cells"] == {g: [g // 4] for g in range(8)}
        assert t["unrated_nodes"] == [] and t["group_of"][40] == 1
        f = lambda x: x.copy().view(np.float32)
        for k in range(KERNELS):
            col, per = t["kernels"][f"kernel_{k:03d}"], t["per_node"]["kernels"][f"kernel_{k:03d}"]
            assert [list(col[p].values()) for p in (0, 1)] == [[float(f(B[p, k, :1])[0])] + B[p, k, 1:].tolist() for p in (0, 1)]
            assert [per[g][g // 4] for g in range(8)] == [{"median": float(f(A[g, k, :1])[0]), "ranks": int(A[g, k, 1])} for g in range(8)]
        for recs, shown in ((Cb, t["node_scores"]), (D, t["ranks"])):
            for i in range(recs.shape[0]):
                d = shown[i]["gpu"]
                assert [d["pace"], d["spread"]] == f(recs[i, 0, :2]).tolist() and [d["columns"], d["slower"], d["faster"]] == recs[i, 0, 2:5].tolist()
        assert [t["ranks"][r]["gpu"]["excess_us"] for r in range(RANKS)] == f(D[:, 0, 7]).tolist()
        slow = t["node_scores"][5]
        assert 0.95 < slow["gpu"]["pace"] < 0.97 and slow["gpu"]["slower"] == KERNELS and slow["members_off_pace"] == PER_NODE
