"""Every route of the score dispatch on the GPU (``nvrx_score_route``: SINGLE, ROWS, ROWS_PRE, TILE16, TILE8) against the C
oracle, on the shapes and tables of tests/score_cases.py.  Every test first asserts the route of the workspace's own result
arrays: a test that believes it is on ROWS but runs SINGLE fails."""
import numpy as np
import pytest
import torch

import score_cases as sc
import synth
from oracle import oracle
from score_cases import ROWS, ROWS_PRE, THRESHOLDS, TILE8, TILE16
from util import close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    from nvrx_straggler.backend import get_backend

    return get_backend()


def _assert_route(be, ws, route):
    """The route of BOTH result blocks of the workspace (successive reports alternate between them)."""
    for blk in ws.blocks:
        got = be.lib.nvrx_score_route(ws.R, ws.K, ws.S, blk.d_scores, blk.d_flags)
        assert got == route, ((ws.R, ws.K, ws.S), sc.ROUTE_NAMES.get(got, got), sc.ROUTE_NAMES[route])


def _workspace(be, T, K, S, route, stats_rows=0):
    R = T.shape[0]
    ws = be.workspace(R, K, S, R, stats_rows)
    _assert_route(be, ws, route)
    ws.send.copy_(torch.from_numpy(T))
    torch.cuda.current_stream().synchronize()  # the copy ran on torch's stream, the score kernels run on the backend's
    return ws


def _check(ws, T, K, S, do_indiv, do_rel):
    """The workspace's current result against the oracle: scores, every flag, meta[:4].  Returns the largest relative
    GPU-score difference."""
    R = T.shape[0]
    exp = oracle.score_table(T, K, S, do_indiv, do_rel)
    worst = sc.compare_scores(ws.scores.copy(), exp)
    # no oracle GPU score sits within 4e-6 of its threshold (tests/test_score_routes_host.py): every flag is decided
    assert np.array_equal(ws.flags, sc.expected_flags(exp, S)), np.argwhere(ws.flags != sc.expected_flags(exp, S))[:8]
    assert list(ws.meta[:4]) == [int((T[:, -1] > 0).all()), R, K, S]
    assert ws.meta[4] == ws.seq
    return worst


@pytest.mark.parametrize("kind", sc.TABLE_KINDS)
@pytest.mark.parametrize("R,K,S", list(sc.ROUTE_SHAPES))
def test_every_route_matches_the_oracle(be, R, K, S, kind):
    """Section columns bit-identical (NaN by NaN-ness, infinities by value and sign), GPU-score columns the same NaN-ness and
    infiniteness and within 2e-6 where finite (f64 sums of non-negative terms in another order), every flag, meta."""
    route = sc.ROUTE_SHAPES[(R, K, S)]
    T = sc.case_table(kind, R, K, S)
    ws = _workspace(be, T, K, S, route)
    worst = 0.0
    for do_indiv, do_rel in sc.COMBOS:
        be.score(ws, ws.send, do_indiv, do_rel, THRESHOLDS)
        worst = max(worst, _check(ws, T, K, S, do_indiv, do_rel))
    print(f"route {sc.ROUTE_NAMES[route]} {(R, K, S)} {kind}: largest relative GPU-score difference {worst:.3g} (bound {sc.GPU_SCORE_RTOL:g})")


# one or two shapes per route; with 1000 rows (2000 16-byte units) the copy loops of k_score (stride R * 256), k_score_tile
# (tiles * 256) and k_score1 (1024) all go round more than once on at least one of them
_STATS_SHAPES = [(64, 0, 94), (1, 0, 12288), (64, 0, 95), (1, 0, 12289), (65, 3, 614), (65, 3, 306), (65, 3, 307)]


@pytest.mark.parametrize("stats_rows", [1, 1000])
@pytest.mark.parametrize("R,K,S", _STATS_SHAPES)
def test_statistics_rows_are_forwarded_on_every_route(be, R, K, S, stats_rows):
    """The score kernels copy the local statistics rows next to the scores: bit patterns (NaN payloads included) arrive
    unchanged under meta[5], and scores and flags are those of the run without statistics."""
    route = sc.ROUTE_SHAPES[(R, K, S)]
    T = sc.case_table("edge_common", R, K, S)
    ws0 = _workspace(be, T, K, S, route)
    be.score(ws0, ws0.send, True, True, THRESHOLDS)
    _check(ws0, T, K, S, True, True)
    scores0, flags0 = ws0.scores.tobytes(), ws0.flags.tobytes()

    rng = np.random.default_rng([R, K, S, stats_rows])
    bits = rng.integers(0, 2**32, size=(stats_rows, 8), dtype=np.uint32)
    bits[0, :3] = (0x7FC12345, 0x7F800001, 0xFFFFFFFF)  # quiet / signalling NaNs with payloads
    bits[-1, -3:] = (0xFFC00001, 0x80000000, 0x00000001)
    ws = _workspace(be, T, K, S, route, stats_rows)
    ws.stats_dev.view(torch.int32).copy_(torch.from_numpy(bits.view(np.int32)))
    torch.cuda.current_stream().synchronize()
    be.score(ws, ws.send, True, True, THRESHOLDS)
    assert ws.meta[5] == ws.seq and ws.meta[4] == ws.seq
    assert np.array_equal(ws.stats.view(np.uint32), bits)
    assert ws.scores.tobytes() == scores0 and ws.flags.tobytes() == flags0
    assert list(ws.meta[:4]) == [0, R, K, S]


@pytest.mark.parametrize("R,K,S", [(64, 0, 95), (65, 3, 614), (100, 7, 9), (65, 3, 307)])
def test_completion_word_on_the_multi_workgroup_routes(be, R, K, S):
    """k_score / k_score_tile publish the sequence word from the LAST workgroup's ticket, after every workgroup's
    system-scope fence, and reset the ticket counter for the next launch.  Two tables with different answers go through
    one workspace, 2000 launches, each checked the instant the word arrives: the whole head (meta, scores, flags, padding)
    must be that table's first result byte for byte -- a counter that is not reset, or a word published before another
    workgroup's rows landed, shows as a stale row.  (The tables change every SECOND launch: the workspace alternates
    between two result blocks, so each block sees both tables in turn.)"""
    route = sc.ROUTE_SHAPES[(R, K, S)]
    assert route in (ROWS, ROWS_PRE, TILE16, TILE8)
    rng = np.random.default_rng([5, R, K, S])
    tabs = [sc.random_table(rng, R, K, S, p_missing=0.0) for _ in range(2)]
    tabs[1][:, : K + S] *= 3.0  # every median differs -> every individual score differs
    exp = [oracle.score_table(t, K, S, True, True) for t in tabs]
    assert not np.array_equal(exp[0][:, 2 : 2 + S], exp[1][:, 2 : 2 + S])
    dev = [torch.from_numpy(t).cuda() for t in tabs]
    ws = be.workspace(R, K, S, R, 0)
    _assert_route(be, ws, route)
    torch.cuda.synchronize()
    W = 2 + 2 * S
    first = [None, None]
    for i in range(2000):
        t = (i >> 1) & 1
        be.score(ws, dev[t], True, True, (0.75, 0.75, 0.75, 0.75))
        head = ws.host_head()
        assert ws.meta[4] == ws.seq and ws.meta[5] == ws.seq, i
        head[16:24] = 0  # meta[4:6], the sequence words, differ by design
        if first[t] is None:
            first[t] = head
            got = ws.scores.copy()
            assert np.array_equal(got[:, 2:W], exp[t][:, 2:W]), i
            sc.compare_scores(got, exp[t])
            assert list(ws.meta[:4]) == [1, R, K, S]
        else:
            assert np.array_equal(head, first[t]), (i, np.flatnonzero(head != first[t])[:8])
    assert not np.array_equal(first[0], first[1])
    torch.cuda.synchronize()
    assert int(ws.done_counter.item()) == 0


def test_scratch_regrowth_behind_a_launch_nobody_waited_for(be, monkeypatch):
    """The column minima of ROWS_PRE / TILE* live in a per-stream scratch buffer that is freed and reallocated when a
    later launch needs more.  On a stream of its own (so the buffer starts empty): a ROWS_PRE launch nobody waits for,
    straight behind it a TILE16 launch that needs a larger buffer, then both results against the oracle."""
    (R1, K1, S1), (R2, K2, S2) = sc.REGROW_SHAPES

    def need(R, K, S):  # floats: the minima and their per-chunk partials
        return (K + S) * (max(1, min(32, (R + 63) // 64)) + 1)

    assert need(R2, K2, S2) > max(need(R1, K1, S1), 1024)
    stream = torch.cuda.Stream(device=be.device)
    monkeypatch.setattr(be, "_stream_handle", stream.cuda_stream)
    T1, T2 = sc.case_table("edge_common", R1, K1, S1), sc.case_table("edge_common", R2, K2, S2)
    ws1, ws2 = _workspace(be, T1, K1, S1, ROWS_PRE), _workspace(be, T2, K2, S2, TILE16)
    be.score(ws1, ws1.send, True, True, THRESHOLDS, wait=False)
    be.score(ws2, ws2.send, True, True, THRESHOLDS, wait=False)
    be.wait_seq(ws1, ws1.seq)
    be.wait_seq(ws2, ws2.seq)
    _check(ws1, T1, K1, S1, True, True)
    _check(ws2, T2, K2, S2, True, True)
    stream.synchronize()


def test_one_call_report_on_the_rows_route():
    """64 logical ranks x 96 sections folded onto one GPU: as many ranks as `k_score1` takes, but their 64 x 194 staged
    scores do not fit its LDS, so the one-call report scores with `k_score` (one workgroup per rank, column minima in LDS).  Two reports (the second one's individual scores use the minima of both), every score against
    the oracle, flagged sets against the scores -- as test_one_call_report_beyond_the_single_workgroup_scorer checks its
    shapes."""
    from nvrx_straggler import Statistic, _native
    from nvrx_straggler.folded import FoldedJob

    R, S, n = 64, 96, 301
    names = [synth.section_name(s) for s in range(S)]
    job = FoldedJob(total_ranks=R, section_names=names, ring_cap=512, node_name="n")
    try:
        hist = None
        slow = (R - 2, R // 3)
        for t in range(2):
            xs = [synth.stress_samples(r + 1000 * t, S, n, slow_rank=slow[t] + 1000 * t, slow_factor=1.5) for r in range(R)]
            for r in range(R):
                job.load(r, xs[r])
            rep = job.report()
            ws = job.reporter._ring_plan.ws
            assert (ws.R, ws.K, ws.S) == (R, 0, S)
            assert _native.load().nvrx_score_route(R, 0, S, ws.d_scores, ws.d_flags) == ROWS
            med = np.stack([oracle.rows_stats(xs[r], np.full(S, n, dtype=np.uint32))[:, 2] for r in range(R)])
            hist = med if hist is None else np.minimum(hist, med)
            T = np.zeros((R, oracle.table_len(0, S)), dtype=np.float32)
            T[:, :S], T[:, S : 2 * S], T[:, -1] = med, hist, 1.0
            exp = oracle.score_table(T, 0, S)
            for s, name in enumerate(names):
                rel, ind = rep.section_relative_perf_scores[name], rep.section_individual_perf_scores[name]
                assert list(rel) == list(range(R))
                for r in range(R):
                    assert close(ind[r], exp[r, 2 + s], rel=1e-6), (t, name, r)
                    assert close(rel[r], exp[r, 2 + S + s], rel=1e-6), (t, name, r)
            got = rep.identify_stragglers()
            assert {k: {x.rank for x in v} for k, v in got["straggler_sections_relative"].items()} == \
                {name: {slow[t]} for name in names}
            exp_ind = {name: {r for r in range(R) if exp[r, 2 + s] < 0.75} for s, name in enumerate(names)}
            assert {k: {x.rank for x in v} for k, v in got["straggler_sections_individual"].items()} == \
                {k: v for k, v in exp_ind.items() if v}
            assert rep.local_section_summaries[names[0]][Statistic.NUM] == n
            assert ws.meta[0] == 1
    finally:
        job.close()
