"""GPU parity of the peer-group kernels (``k_peer_cols``, ``k_peer_rank``) and of the peer step of a report against the
NumPy restatement of tests/peer_oracle_backend.py.  Every record and every slot of every case is compared.

Bounds: column records and section slots bit for bit (an actual value, counts and ranks; one f64 quotient rounded to f32);
NaN and inf masks equal; GPU slots within 2e-6 * max(1, |expected|), the tolerance tests/test_gpu_tail.py and
tests/test_gpu_robust.py use for the same f64 weighted mean summed in another order."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import peer_workers
from mp_util import run_ranks
from peer_oracle_backend import STAGE_SLOW_RANK, peer_group_arrays, peer_scores_table
from test_gpu_score import _random_table

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# K+S either side of a 64-column tile; fewer ranks than waves, more; more than one block either way; the largest R and K
SHAPES = [(1, 3, 0), (2, 2, 2), (5, 4, 4), (8, 0, 63), (8, 0, 64), (8, 1, 64), (9, 5, 6), (64, 17, 33), (65, 0, 64), (100, 7, 9),
          (4096, 32, 16), (8, 4096, 8)]
SPECIALS = ("full", "single", "equal", "zero_inf", "group_lacks")


@pytest.fixture(scope="module")
def be():
    from nvrx_straggler.backend import get_backend

    return get_backend()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _groupings(R):
    """``(name, labels)`` of the issue's groupings, where they fit ``R`` ranks."""
    out = [("one", [0] * R), ("block:4", [r // 4 for r in range(R)])]
    if R >= 3:
        out.append(("mod:3", [r % 3 for r in range(R)]))  # interleaved, sizes differ by one
    if 1 < R <= 4096:
        out.append(("singletons", list(range(R))))
    if R >= 15:
        # sizes 1, 2, 3, 4, 5 (fewer members than waves, exactly four, more) and the rest, interleaved over the ranks
        labels = sum(([g] * (g + 1) for g in range(5)), []) + [5] * (R - 15)
        out.append(("hand-made", np.random.default_rng(R).permutation(labels).tolist()))
    return out


def _special(T, rng, c, kind, K, S, group):
    """Rewrite column ``c`` of the table's med part (and, for a kernel column, its weights) as one of the issue's columns."""
    R, KS = T.shape[0], K + S
    col = np.full(R, -1.0, dtype=np.float32)
    if kind == "full":  # a column nobody misses
        col[:] = rng.lognormal(1.0, 0.5, R)
    elif kind == "single":  # present on a single rank
        col[rng.integers(R)] = np.float32(rng.lognormal(1.0, 0.5))
    elif kind == "equal":  # all members equal: the lowest rank of every group is its floor_rank
        col[:] = np.float32(3.25)
    elif kind == "zero_inf":  # a 0.0 and a +inf among ordinary values
        col[:] = rng.lognormal(1.0, 0.5, R)
        col[rng.random(R) < 0.15] = -1.0
        col[0] = 0.0
        col[R - 1] = np.inf if R > 1 else 0.0
    elif kind == "group_lacks":  # a column that one whole group lacks
        col[:] = rng.lognormal(1.0, 0.5, R)
        col[np.asarray(group) == group[rng.integers(R)]] = -1.0
    T[:, c] = col
    if c < K:
        T[:, 2 * KS + c] = np.where(col >= 0, rng.uniform(1, 1000, R), 0.0).astype(np.float32)


def _tables(R, K, S, group):
    """``_random_table`` with 15 % of the medians absent plus the special columns, spread over the columns (a case with fewer
    columns than special ones gets several tables, so that each is exercised)."""
    rng = np.random.default_rng(R * 1000 + K + S)
    KS = K + S
    todo = list(SPECIALS)
    while todo:
        T = _random_table(rng, R, K, S)
        take, todo = todo[:KS], todo[KS:]
        cols = np.linspace(0, KS - 1, len(take)).astype(int) if len(take) > 1 else [KS // 2]
        for c, kind in zip(cols, take):
            _special(T, rng, int(c), kind, K, S, group)
        yield T


def _run(be, T, K, S, arrays, G, first_rank, n_ranks, min_ranks):
    from nvrx_straggler.backend import PeerGroups

    R = T.shape[0]
    groups = PeerGroups(arrays[:R].tolist())
    assert groups.G == G and np.array_equal(groups.host, arrays)
    ws = be.workspace(R, K, S, R, 0)
    ws.peer_settle()
    ws.send.copy_(torch.from_numpy(T))
    torch.cuda.synchronize()
    return be.peer_score(ws, ws.send, groups, first_rank, n_ranks, min_ranks).records()


def _compare(got, exp, tag):
    (gcols, gsc), (ecols, esc) = got, exp
    assert gcols.shape == ecols.shape and gsc.shape == esc.shape, tag
    bad = np.argwhere((gcols != ecols).any(axis=2))
    assert bad.size == 0, (tag, "records (group, column)", bad[:8].tolist(), gcols[tuple(bad[:4].T)], ecols[tuple(bad[:4].T)])
    assert np.array_equal(np.isnan(gsc), np.isnan(esc)), (tag, "NaN masks", np.argwhere(np.isnan(gsc) != np.isnan(esc))[:8])
    assert np.array_equal(np.isposinf(gsc), np.isposinf(esc)) and np.array_equal(np.isneginf(gsc), np.isneginf(esc)), (tag, "inf masks")
    sec_g, sec_e = gsc[:, 1:], esc[:, 1:]
    bad = np.argwhere(~np.isnan(sec_e) & (_bits(sec_g) != _bits(sec_e)))
    assert bad.size == 0, (tag, "sections", bad[:8].tolist(), sec_g[tuple(bad[:8].T)], sec_e[tuple(bad[:8].T)])
    g, e = gsc[:, 0].astype(np.float64), esc[:, 0].astype(np.float64)
    fin = np.isfinite(e)
    if fin.any():
        err = np.abs(g[fin] - e[fin]) / np.maximum(1.0, np.abs(e[fin]))
        print(tag, "GPU slots: max error", float(err.max()), "of", int(fin.sum()))
        assert err.max() <= 2e-6, (tag, "GPU slots", float(err.max()))


@pytest.mark.parametrize("R,K,S", SHAPES)
def test_peer_score_matches_numpy(be, R, K, S):
    for name, labels in _groupings(R):
        arrays, names = peer_group_arrays(labels)
        G = len(names)
        for t, T in enumerate(_tables(R, K, S, labels)):
            for min_ranks in (1, 2, 4):
                tag = (R, K, S, name, t, min_ranks)
                got = _run(be, T, K, S, arrays, G, 0, R, min_ranks)
                _compare(got, peer_scores_table(T, K, S, arrays, G, 0, R, min_ranks), tag)
                if min_ranks == 2 and R > 1:
                    # a sub-range of ranks (first_rank > 0) equals the slice of the full result, bit for bit
                    lo, n = max(1, R // 3), max(1, R // 2)
                    pcols, psc = _run(be, T, K, S, arrays, G, lo, n, min_ranks)
                    assert np.array_equal(pcols, got[0]) and np.array_equal(_bits(psc), _bits(got[1][lo : lo + n])), tag


@pytest.mark.parametrize("R,K,S", [(1, 3, 2), (8, 0, 64), (9, 5, 6), (65, 3, 64), (100, 7, 9)])
def test_one_group_and_one_rank_minimum_give_the_relative_section_scores(be, R, K, S):
    """The section slots are the relative section scores ``be.score`` writes for the same table, bit for bit: everywhere on
    a table without absent medians, and on ``_random_table`` (15 % absent) in every section that every rank has.  A section
    that some rank lacks has no job-wide reference at all (the -1 sentinel wins the minimum: reporting.py:255-296), while
    the peer scores rate the ranks that have it, as the contract's "present" says -- those slots are compared with the
    restatement in ``test_peer_score_matches_numpy``."""
    rng = np.random.default_rng(R + K + S)
    arrays, _ = peer_group_arrays([0] * R)
    for full in (True, False):
        T = _random_table(rng, R, K, S)
        if full:
            T[:, K : K + S] = rng.lognormal(1.0, 0.5, (R, S)).astype(np.float32)
        ws = be.workspace(R, K, S, R, 0)
        ws.peer_settle()
        ws.send.copy_(torch.from_numpy(T))
        be.score(ws, ws.send, False, True, (0.75, 0.75, 0.75, 0.75))
        rel = ws.scores[:, 2 + S : 2 + 2 * S].copy()
        _, sc = _run(be, T, K, S, arrays, 1, 0, R, 1)
        with np.errstate(invalid="ignore"):
            complete = (T[:, K : K + S] >= 0).all(axis=0)
        assert complete.all() or not full
        assert not np.isnan(rel[:, complete]).any() and np.isnan(rel[:, ~complete]).all()
        assert np.array_equal(_bits(sc[:, 1:][:, complete]), _bits(rel[:, complete])), (R, K, S, full)


def test_out_of_range_group_contents_are_guarded(be):
    """A group id of G, a member of R, a ``start`` beyond R (and negative ones): NaN slots and skipped members as the
    restatement says, and no word outside NVRX_PEER_WORDS of a guard-padded buffer is touched.  Valid launches only: the
    kernels' guards keep every access inside the table, the array and the buffer."""
    from nvrx_straggler import _native

    R, K, S, G, PAD, FILL = 21, 5, 70, 4, 64, 0x5A5A5A5A
    rng = np.random.default_rng(77)
    T = _random_table(rng, R, K, S)
    labels = [r % G for r in range(R)]
    good, _ = peer_group_arrays(labels)
    cases = {"intact": good.copy()}
    a = cases["group id G and -1"] = good.copy()
    a[3], a[8] = G, -1
    a = cases["member R and -1"] = good.copy()
    a[R + 2], a[R + 9] = R, -1
    a = cases["start beyond R"] = good.copy()
    a[2 * R + G] = R + 5
    a = cases["start below 0 and descending"] = good.copy()
    a[2 * R], a[2 * R + 2] = -3, 1
    a = cases["everything"] = good.copy()
    a[0], a[R + R - 1], a[2 * R + G], a[2 * R + 1] = G + 7, 1 << 30, 1 << 30, -(1 << 30)
    table = torch.from_numpy(T).cuda()
    for name, arrays in cases.items():
        for first, n in ((0, R), (4, 9)):
            words = _native.peer_words(G, n, K, S)
            out = torch.full((PAD + words + PAD,), FILL, dtype=torch.int32, device="cuda")
            d_groups = torch.from_numpy(arrays).cuda()
            torch.cuda.synchronize()
            rc = be.lib.nvrx_peer_score(table.data_ptr(), R, K, S, d_groups.data_ptr(), G, first, n, 2,
                                        out.data_ptr() + 4 * PAD, be._stream_handle)
            assert rc == 0, (name, be.lib.nvrx_last_error())
            be.synchronize()
            torch.cuda.synchronize()
            host = out.cpu().numpy().view(np.uint32)
            assert (host[:PAD] == FILL).all() and (host[PAD + words :] == FILL).all(), name
            body = host[PAD : PAD + words]
            got = (body[: 4 * G * (K + S)].reshape(G, K + S, 4), body[4 * G * (K + S) :].view(np.float32).reshape(n, 1 + S))
            exp = peer_scores_table(T, K, S, arrays, G, first, n, 2)
            _compare(got, exp, (name, first, n))
            if name == "group id G and -1" and first == 0:
                assert np.isnan(got[1][3]).all() and np.isnan(got[1][8]).all() and not np.isnan(got[1][4]).all()
            if name == "start beyond R":
                assert got[0][G - 1, 0, 3] == R - int(good[2 * R + G - 1])  # clamped to R


def test_argument_errors_come_back_before_the_device_is_touched(be):
    import ctypes

    from nvrx_straggler import _native

    lib = be.lib
    R, K, S, G = 8, 8, 2, 2
    table = torch.zeros((R, _native.table_len(K, S)), dtype=torch.float32, device="cuda")
    groups = torch.from_numpy(peer_group_arrays([r // 4 for r in range(R)])[0]).cuda()
    out = torch.full((_native.peer_words(G, R, K, S),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def score(tp=table.data_ptr(), R=R, gp=groups.data_ptr(), G=G, first=0, n=R, min_ranks=2, op=out.data_ptr()):
        return lib.nvrx_peer_score(tp, R, K, S, gp, G, first, n, min_ranks, op, be._stream_handle)

    assert score(tp=None) == _native.ERR_INVALID and score(op=None) == _native.ERR_INVALID and score(gp=None) == _native.ERR_INVALID
    assert score(R=_native.ROBUST_MAX_RANKS + 1, n=1) == _native.ERR_RANGE
    assert score(first=7, n=2) == _native.ERR_RANGE and score(first=-1) == _native.ERR_RANGE and score(n=R + 1) == _native.ERR_RANGE
    assert score(min_ranks=0) == _native.ERR_RANGE
    assert score(G=0) == _native.ERR_INVALID and score(G=R + 1) == _native.ERR_RANGE
    assert score(op=out.data_ptr() + 4) == _native.ERR_INVALID
    desc = _native.ReportDesc()
    desc.R, desc.K, desc.S = R, K, S
    assert lib.nvrx_report_peer(None, ctypes.byref(desc), groups.data_ptr(), G, 0, R, 2, out.data_ptr()) == _native.ERR_INVALID
    be.synchronize()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x5A5A5A5A).all()  # nothing was launched


# ---- the peer step of a report --------------------------------------------------------------------------------------------
def _expected_stage_tables(sections=4):
    """What the restatement says of the two-stage job's table: kernel ids in ``KERNELS``' order, then the sections."""
    from nvrx_straggler import _native

    data, med = peer_workers.stage_samples(sections=sections)
    K, S = len(peer_workers.KERNELS), sections
    T = np.full((8, _native.table_len(K, S)), -1.0, dtype=np.float32)
    T[:, :K], T[:, K : K + S] = med[:, sections:], med[:, :sections]
    n = data.shape[2]
    T[:, 2 * (K + S) : 2 * (K + S) + K] = (n * data[:, sections:].astype(np.float64).mean(axis=2)).astype(np.float32)  # NUM * AVG
    return T, K, S


def _check_stage_reports(reports, ranks, labels=(0, 0, 0, 0, 1, 1, 1, 1), sections=4):
    T, K, S = _expected_stage_tables(sections)
    arrays, names = peer_group_arrays(list(labels))
    cols, sc = peer_scores_table(T, K, S, arrays, len(names), ranks[0], len(ranks), 2)
    floors = cols[:, :, 0].view(np.float32)
    section_names = [f"section_{s:03d}" for s in range(S)]
    for i, rep in enumerate(reports):
        t = rep["peer"]
        assert sorted(t["gpu_relative"]) == list(ranks) and t["min_ranks"] == 2 and t["unrated_ranks"] == [], i
        assert t["groups"] == {lab: [r for r in range(8) if labels[r] == lab] for lab in names}
        assert t["group_of"] == {r: labels[r] for r in ranks}
        assert sorted(t["section_relative"]) == section_names and sorted(t["kernel_floor"]) == sorted(peer_workers.KERNELS)
        for j, r in enumerate(ranks):
            g, e = t["gpu_relative"][r], float(sc[j, 0])
            assert abs(g - e) <= 2e-6 * max(1.0, abs(e)), (i, r, g, e)  # (also covers the f32 weights NUM * AVG)
            for s, n in enumerate(section_names):
                assert t["section_relative"][n][r] == float(sc[j, 1 + s]), (i, r, n)
        for s, n in enumerate(section_names):
            for g, lab in enumerate(names):
                assert t["section_floor"][n][lab] == float(floors[g, K + s]) and t["ranks_with_data"][n][lab] == 4
                assert t["section_fastest"][n][lab] == int(cols[g, K + s, 2])
        for k, n in enumerate(peer_workers.KERNELS):
            for g, lab in enumerate(names):
                assert t["kernel_floor"][n][lab] == float(floors[g, k]), (i, n, lab)
        if len(ranks) == 8:
            assert rep["job_flagged"] == [4, 5, 6, 7] and rep["peer_flagged"] == [STAGE_SLOW_RANK], (i, rep["job_flagged"], rep["peer_flagged"])


@pytest.mark.parametrize("asynchronous", [False, True])
def test_report_step_on_the_general_and_the_one_call_path(be, asynchronous):
    torch.cuda.set_device(0)
    reports = peer_workers.folded_stages(0, 1, asynchronous=asynchronous)
    assert [r["fused"] for r in reports] == [False, True, True]  # the general path, then the one-call report
    _check_stage_reports(reports, range(8))


def test_report_step_behind_a_report_that_was_scored_resident():
    """``nvrx_report_peer``'s ordering: the score kernel ran on a stream of its own, the peer kernels follow it by an event."""
    res = run_ranks(peer_workers.folded_stages_sync_then_async, 1, timeout=300, use_oracle_backend=False, device=0,
                    env={"NVRX_DEBUG_RESIDENT_SCORER": "2"})[0]
    for mode in ("sync", "async"):
        assert [r["fused"] for r in res[mode]] == [False, True, True], mode
        _check_stage_reports(res[mode], range(8))


def test_two_processes_sharing_the_gpu_on_the_stepwise_path():
    """Default route (gloo / c10d): the planned report is three calls with a collective between them; both ranks hold reports
    of their own four logical ranks, the groups given as labels."""
    labels = ["first"] * 4 + ["second"] * 4
    res = run_ranks(peer_workers.folded_stages, 2, timeout=420, use_oracle_backend=False, device=0, gather_on_rank0=False,
                    peer_groups=labels)
    for rank in range(2):
        assert [r["fused"] for r in res[rank]] == [False, False, False]
        _check_stage_reports(res[rank], range(4 * rank, 4 * rank + 4), labels=labels)


def test_the_example_names_rank_6_by_its_peers_and_four_ranks_by_the_job():
    out = subprocess.run([sys.executable, os.path.join(REPO, "examples", "straggler_example.py"), "--peer"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    job = re.search(r"identify_stragglers\(\): (\[[^\]]*\])", out.stdout)
    peers = re.search(r"identify_peer_stragglers\(\): (\[[^\]]*\])", out.stdout)
    assert job and peers, out.stdout
    assert job.group(1) == "[4, 5, 6, 7]" and peers.group(1) == "[6]", out.stdout
