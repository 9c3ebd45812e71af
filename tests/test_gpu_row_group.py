"""GPU parity of the row families' score step per peer group (``nvrx_rowfam_group_score``: ``k_peer_cols`` on plane 0,
``k_rowfam_group_rank``) against the NumPy restatement of tests/row_group_oracle_backend.py, against the entries it must agree
with (``nvrx_peer_score``, ``nvrx_tail_score``), and of a report's grouped steps against the CPU checker's report.

Through the C ABI into a guard-padded buffer: 64 words of fill either side, unchanged afterwards; the inputs are read only.
Bounds: block A and the section slots bit for bit (an actual value, counts and ranks; one f64 quotient rounded to f32); NaN and
inf masks equal; GPU slots within 2e-6 * max(1, |expected|), the bound tests/test_gpu_tail.py and tests/test_gpu_peer.py use for
this f64 weighted mean summed in another order."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import row_group_oracle_backend as rg
import row_group_workers
from mp_util import run_ranks
from peer_oracle_backend import peer_group_arrays
from row_group_oracle_backend import FAMILY_NAMES, RowGroupOracleBackend, row_group_records
from score_cases import random_table
from test_gpu_peer import _bits, _compare, _groupings, _tables
from test_row_group_host import KERNELS, PARENT_KEYS

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# K+S either side of a 64-column tile, K either side of a workgroup's 256 threads; fewer ranks than waves, more
SHAPES = [(1, 3, 0), (2, 2, 2), (5, 4, 4), (8, 0, 63), (8, 0, 64), (8, 1, 64), (8, 255, 1), (8, 256, 0), (8, 257, 257),
          (64, 17, 33), (65, 0, 64), (100, 7, 9)]
PLANE_COUNTS = (1, 6, 7)
PAD, FILL = 64, 0x5A5A5A5A
POISON = np.float32(1e-20)  # planes 1..: present and below every value -- a floor, were it ever read


@pytest.fixture(scope="module")
def be():
    from nvrx_straggler.backend import get_backend

    return get_backend()


def _planes_of(T, KS, P):
    """``[R, P, KS]``: plane 0 the table's med part, the others poison."""
    out = np.full((T.shape[0], P, KS), POISON, dtype=np.float32)
    out[:, 0, :] = T[:, :KS]
    return out


def _score(be, planes, T, K, S, arrays, G, first, n, min_ranks):
    """One call through the C ABI; ``(cols, scores)`` of the body, the guards and the inputs checked."""
    from nvrx_straggler import _native

    R, P, KS = planes.shape
    words = _native.rowfam_group_words(G, K, S, n)
    assert words == be.lib.nvrx_rowfam_group_words(G, K, S, n)
    d_planes = torch.from_numpy(planes).cuda()
    d_table = torch.from_numpy(T).cuda() if K > 0 else None
    d_groups = torch.from_numpy(arrays).cuda()
    out = torch.full((PAD + words + PAD,), FILL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = be.lib.nvrx_rowfam_group_score(d_planes.data_ptr(), P, d_table.data_ptr() if d_table is not None else None, R, K, S,
                                        d_groups.data_ptr(), G, first, n, min_ranks, out.data_ptr() + 4 * PAD, be._stream_handle)
    assert rc == 0, be.lib.nvrx_last_error()
    be.synchronize()
    torch.cuda.synchronize()
    host = out.cpu().numpy().view(np.uint32)
    assert (host[:PAD] == FILL).all() and (host[PAD + words:] == FILL).all(), "a word outside the block was written"
    assert np.array_equal(_bits(d_planes.cpu().numpy()), _bits(planes)) and np.array_equal(d_groups.cpu().numpy(), arrays)
    assert d_table is None or np.array_equal(_bits(d_table.cpu().numpy()), _bits(T))
    body = host[PAD : PAD + words]
    return body[: 4 * G * KS].reshape(G, KS, 4).copy(), body[4 * G * KS:].view(np.float32).reshape(n, 1 + S).copy()


# ---- 1. the entry against the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("R,K,S", SHAPES)
def test_rowfam_group_score_matches_numpy(be, R, K, S):
    KS = K + S
    for name, labels in _groupings(R):
        arrays, names = peer_group_arrays(labels)
        G = len(names)
        for t, T in enumerate(_tables(R, K, S, labels)):
            for min_ranks in (1, 2):
                exp = row_group_records(T[:, :KS], T, K, S, arrays, G, 0, R, min_ranks)
                full = None
                for P in PLANE_COUNTS:
                    tag = (R, K, S, name, t, min_ranks, P)
                    got = _score(be, _planes_of(T, KS, P), T, K, S, arrays, G, 0, R, min_ranks)
                    _compare(got, exp, tag)
                    if full is not None:  # the pitch changes nothing, to the bit
                        assert np.array_equal(got[0], full[0]) and np.array_equal(_bits(got[1]), _bits(full[1])), tag
                    full = got
                if min_ranks == 2 and R > 1:
                    # a sub-range of ranks (first_rank > 0) equals the slice of the full result, bit for bit
                    lo, n = max(1, R // 3), max(1, R // 2)
                    pcols, psc = _score(be, _planes_of(T, KS, 6), T, K, S, arrays, G, lo, n, min_ranks)
                    assert np.array_equal(pcols, full[0]) and np.array_equal(_bits(psc), _bits(full[1][lo : lo + n])), (R, K, S, name, t)


def test_out_of_range_group_contents_are_guarded(be):
    """A group id of G, a member of R, a ``start`` beyond R (and negative ones): NaN slots and skipped members as the
    restatement says, and no word outside the block of a guard-padded buffer is touched.  Valid launches only: the kernels'
    guards keep every access inside the inputs and the buffer."""
    R, K, S, G = 21, 5, 70, 4
    T = random_table(np.random.default_rng(78), R, K, S)
    good, _ = peer_group_arrays([r % G for r in range(R)])
    hostile = good.copy()
    hostile[0], hostile[3], hostile[8] = G + 7, G, -1                      # group ids outside [0, G)
    hostile[R + 2], hostile[R + 9], hostile[2 * R - 1] = R, -1, 1 << 30    # members outside [0, R)
    hostile[2 * R + G], hostile[2 * R + 1] = 1 << 30, -(1 << 30)           # starts outside [0, R]
    for name, arrays in (("intact", good), ("hostile", hostile)):
        for first, n in ((0, R), (4, 9)):
            for P in (1, 7):
                got = _score(be, _planes_of(T, K + S, P), T, K, S, arrays, G, first, n, 2)
                _compare(got, row_group_records(T[:, : K + S], T, K, S, arrays, G, first, n, 2), (name, first, n, P))
                if name == "hostile" and first == 0:
                    # (group 0's stretch is empty behind the clamped start: rank 4 is unrated too; group 1's is not)
                    assert all(np.isnan(got[1][r]).all() for r in (0, 3, 4, 8)) and not np.isnan(got[1][5]).all()


# ---- 2. against the entries it must agree with ------------------------------------------------------------------------------
@pytest.mark.parametrize("R,K,S", [(5, 4, 4), (8, 257, 257), (65, 0, 64), (100, 7, 9)])
def test_on_the_tables_med_part_it_is_the_peer_score(be, R, K, S):
    """Plane 0 = the table's med part: block A equals ``nvrx_peer_score``'s column records word for word, the section slots
    bit for bit."""
    from nvrx_straggler import _native

    KS = K + S
    for name, labels in _groupings(R):
        arrays, names = peer_group_arrays(labels)
        G = len(names)
        T = next(iter(_tables(R, K, S, labels)))
        words = _native.peer_words(G, R, K, S)
        d_table, d_groups = torch.from_numpy(T).cuda(), torch.from_numpy(arrays).cuda()
        out = torch.full((words,), FILL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert be.lib.nvrx_peer_score(d_table.data_ptr(), R, K, S, d_groups.data_ptr(), G, 0, R, 2, out.data_ptr(), be._stream_handle) == 0
        be.synchronize()
        peer = out.cpu().numpy().view(np.uint32)
        pcols, psc = peer[: 4 * G * KS].reshape(G, KS, 4), peer[4 * G * KS:].view(np.float32).reshape(R, 1 + S)
        for P in (1, 6):
            cols, sc = _score(be, _planes_of(T, KS, P), T, K, S, arrays, G, 0, R, 2)
            assert np.array_equal(cols, pcols), (R, K, S, name, P)
            assert np.array_equal(_bits(sc[:, 1:]), _bits(psc[:, 1:])), (R, K, S, name, P)


@pytest.mark.parametrize("R,K,S", [(2, 2, 2), (8, 1, 64), (65, 0, 64), (100, 7, 9)])
def test_one_group_of_full_columns_gives_the_tail_scores_section_slots(be, R, K, S):
    """One group of all ranks, ``min_ranks = 1``, every rank holding every column: the section slots are ``nvrx_tail_score``'s,
    bit for bit (the job-wide rule and the grouped one part only where a rank lacks a column)."""
    KS = K + S
    T = random_table(np.random.default_rng(R + K + S), R, K, S, p_missing=0.0)
    tails = np.ascontiguousarray(T[:, :KS])
    d_tails, d_table = torch.from_numpy(tails).cuda(), torch.from_numpy(T).cuda()
    scratch = torch.zeros(max(33 * KS, 64), dtype=torch.float32, device="cuda")
    out = torch.zeros((R, 1 + S), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert be.lib.nvrx_tail_score(d_tails.data_ptr(), d_table.data_ptr(), R, K, S, 0, R, scratch.data_ptr(), out.data_ptr(),
                                  be._stream_handle) == 0
    be.synchronize()
    want = out.cpu().numpy()
    arrays, _ = peer_group_arrays([0] * R)
    for P in PLANE_COUNTS:
        _, sc = _score(be, _planes_of(T, KS, P), T, K, S, arrays, 1, 0, R, 1)
        assert not np.isnan(sc[:, 1:]).any() and np.array_equal(_bits(sc[:, 1:]), _bits(want[:, 1:])), (R, K, S, P)
        fin = np.isfinite(want[:, 0])
        assert np.array_equal(fin, np.isfinite(sc[:, 0]))
        if fin.any():
            assert (np.abs(sc[fin, 0].astype(np.float64) - want[fin, 0]) / np.maximum(1.0, np.abs(want[fin, 0]))).max() <= 2e-6


def test_argument_errors_come_back_before_the_device_is_touched(be):
    from nvrx_straggler import _native

    R, K, S, G, P = 8, 8, 2, 2, 7
    planes = torch.zeros((R, P * (K + S)), dtype=torch.float32, device="cuda")
    table = torch.zeros((R, _native.table_len(K, S)), dtype=torch.float32, device="cuda")
    groups = torch.from_numpy(peer_group_arrays([r // 4 for r in range(R)])[0]).cuda()
    out = torch.full((_native.rowfam_group_words(G, K, S, R),), FILL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def score(pp=planes.data_ptr(), P=P, tp=table.data_ptr(), R=R, gp=groups.data_ptr(), G=G, first=0, n=R, min_ranks=2,
              op=out.data_ptr()):
        return be.lib.nvrx_rowfam_group_score(pp, P, tp, R, K, S, gp, G, first, n, min_ranks, op, be._stream_handle)

    INVALID, RANGE = _native.ERR_INVALID, _native.ERR_RANGE
    assert score(pp=None) == INVALID and score(tp=None) == INVALID and score(gp=None) == INVALID and score(op=None) == INVALID
    assert score(P=0) == RANGE and score(P=8) == RANGE and score(R=_native.ROBUST_MAX_RANKS + 1, n=1) == RANGE
    assert score(first=7, n=2) == RANGE and score(first=-1) == RANGE and score(n=R + 1) == RANGE and score(min_ranks=0) == RANGE
    assert score(G=0) == INVALID and score(G=R + 1) == RANGE and score(op=out.data_ptr() + 4) == INVALID
    be.synchronize()
    torch.cuda.synchronize()
    assert (out.cpu().numpy().view(np.uint32) == FILL).all()  # nothing was launched


# ---- 3. the grouped steps of a report ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle():
    """The reference, computed once: the small exact window on the CPU checker -- three windows with the option on, the first
    with it off."""
    from nvrx_straggler import backend

    before, cpu = backend._backend, RowGroupOracleBackend()
    backend.set_backend(cpu)
    try:
        gen, rings, rows = rg.make(cpu, KERNELS)
        on = [rg.family_scores(rg.report(gen, rings, rows, KERNELS, w)) for w in range(3)]
        gen.close()
        gen, rings, rows = rg.make(cpu, KERNELS, **rg.OPTIONS)
        off = rg.family_scores(rg.report(gen, rings, rows, KERNELS, 0))
        gen.close()
        return {"on": on, "off": off}
    finally:
        backend.set_backend(before)


def _close(a, b) -> bool:
    """``rg.same`` with the planes' own tolerance for the floats of a rank's record (tests/test_gpu_row_families.py: means
    within an ulp, strengths within 1.2e-7)."""
    if isinstance(a, dict) and isinstance(b, dict):
        return a.keys() == b.keys() and all(_close(a[k], b[k]) for k in a)
    if isinstance(a, float) and isinstance(b, float):
        return (a != a and b != b) or abs(a - b) <= 2.4e-7 * max(1.0, abs(b))
    return rg.same(a, b)


def _check_on(got, want, where):
    records = {"tail": "tails", "onset": "onsets", "period": "periods", "episode": "episodes"}
    for fam in FAMILY_NAMES:
        g, w = got[fam], want[fam]
        assert g.keys() == w.keys() == PARENT_KEYS[fam] | set(rg.NEW_KEYS), (where, fam)
        for key in g:
            if key in ("section_" + records[fam], "kernel_" + records[fam]) and fam != "tail":
                assert _close(g[key], w[key]), (where, fam, key, g[key], w[key])
            else:  # scores, references and the groups: equal
                assert rg.same(g[key], w[key]), (where, fam, key, g[key], w[key])


@pytest.mark.parametrize("asynchronous", [False, True])
def test_the_window_on_the_engine_equals_the_checkers_report(be, oracle, asynchronous):
    """Three windows on one workspace (the general report, then planned ones), the first read only after the next two were
    issued; once with asynchronous reports."""
    gen, rings, rows = rg.make(be, KERNELS, asynchronous=asynchronous)
    try:
        held = [rg.report(gen, rings, rows, KERNELS, w) for w in range(3)]
        for w in (2, 0, 1):
            _check_on(rg.family_scores(held[w]), oracle["on"][w], (asynchronous, w))
        handle_types = {type(held[0].__dict__[s]).__name__ for s in ("_tail", "_onset", "_period", "_episode")}
        assert handle_types == {"dict"}  # read: materialised
    finally:
        gen.close()
        rings.close()


def test_auto_groups_and_the_option_off_on_the_engine(be, oracle):
    from nvrx_straggler.reporting import _RowFamilySource

    gen, rings, rows = rg.make(be, KERNELS, peer_groups="auto")
    try:
        got = rg.family_scores(rg.report(gen, rings, rows, KERNELS, 0))
        for fam in FAMILY_NAMES:
            assert sorted(got[fam]["groups"].values()) == [[0, 1], [2, 3]]
            assert rg.same(got[fam]["section_relative"], oracle["on"][0][fam]["section_relative"]), fam
            assert rg.same(got[fam]["gpu_relative"], oracle["on"][0][fam]["gpu_relative"]), fam
    finally:
        gen.close()
        rings.close()
    calls = []
    inner = be._family_group_score
    be._family_group_score = lambda *a, **kw: calls.append(a) or inner(*a, **kw)
    gen, rings, rows = rg.make(be, KERNELS, **rg.OPTIONS)  # peer_groups and all four families, the option off
    try:
        rep = rg.report(gen, rings, rows, KERNELS, 0)
        assert all(type(rep.__dict__[s]) is _RowFamilySource for s in ("_tail", "_onset", "_period", "_episode")) and not calls
        got = rg.family_scores(rep)
        for fam in FAMILY_NAMES:
            assert got[fam].keys() == PARENT_KEYS[fam] and _close(got[fam], oracle["off"][fam]), fam
            assert rg.same(got[fam]["section_relative"], oracle["off"][fam]["section_relative"]), fam
    finally:
        del be._family_group_score
        gen.close()
        rings.close()


def test_the_buffer_grows_behind_a_settle_when_there_are_more_groups(be):
    """Two label lists on one workspace shape: the second has more groups, the family's buffer grows with the gathered table
    carried over, and a held report of the first keeps its own records."""
    from nvrx_straggler import row_families

    gen, rings, rows = rg.make(be, KERNELS, peer_groups=(0, 0, 0, 0), peer_min_ranks=1)
    gen2 = rings2 = None
    try:
        first = rg.report(gen, rings, rows, KERNELS, 0)
        ws = gen._ring_plan.ws
        before = {f.name: ws._family_state[f.name].buf.numel() for f in row_families.FAMILIES}
        gen2, rings2, rows2 = rg.make(be, KERNELS, peer_groups=(0, 1, 2, 3), peer_min_ranks=1)
        second = rg.report(gen2, rings2, rows2, KERNELS, 1)
        ws2 = gen2._ring_plan.ws
        assert ws2 is ws  # (the cache is per table shape, across generators: were it not, the growth below would check nothing)
        assert all(ws._family_state[f.name].buf.numel() > before[f.name] for f in row_families.FAMILIES)
        t1, t2 = first.tail_scores(), second.tail_scores()
        assert t1["groups"] == {0: [0, 1, 2, 3]} and t2["groups"] == {g: [g] for g in range(4)}
        assert t1["section_relative"]["step"] == {0: 1.0, 1: 1.0, 2: float(np.float32(1000.0 / 1500.0)), 3: float(np.float32(1000.0 / 1500.0))}
        assert t2["section_relative"]["step"] == {r: 1.0 for r in range(4)}
        assert t2["section_reference"]["step"][3] == {"value": 3000.0, "rank": 3, "ranks": 1}
    finally:
        gen.close()
        if gen2 is not None:
            gen2.close()
            rings2.close()
        rings.close()


def test_four_processes_sharing_the_gpu_give_the_folded_report(be):
    """One logical rank per process, ``block:2``: rank 0 gathers and scores per group, the others run the local kernels and
    the all-gathers only.  The grouped scores are those of the folded single-process run on the same engine."""
    gen, rings, rows = rg.make(be, KERNELS, peer_groups="block:2")
    try:
        folded = [rg.family_scores(rg.report(gen, rings, rows, KERNELS, w)) for w in range(2)]
    finally:
        gen.close()
        rings.close()
    res = run_ranks(row_group_workers.window_reports, 4, timeout=420, use_oracle_backend=False, device=0)
    assert all(r["reports"] == [None, None] for r in res[1:])
    for w, got in enumerate(res[0]["reports"]):
        for fam in FAMILY_NAMES:
            assert rg.same(got[fam], folded[w][fam]), (w, fam, got[fam], folded[w][fam])


@pytest.mark.parametrize("mode,job_wide,grouped", [("tail", "[4, 5, 6, 7]", "[6]"), ("period", "[2, 4, 5, 6, 7]", "[2]")])
def test_the_example_names_one_rank_per_group_and_a_whole_stage_job_wide(mode, job_wide, grouped):
    out = subprocess.run([sys.executable, os.path.join(REPO, "examples", "straggler_example.py"), f"--{mode}-peer"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    found = dict(re.findall(rf"identify_{mode}_stragglers\(\) with row_peer_groups=(False|True): (\[[^\]]*\])", out.stdout))
    assert found == {"False": job_wide, "True": grouped}, out.stdout
    if mode == "tail":
        assert re.findall(r"identify_peer_stragglers\(\): (\[[^\]]*\])", out.stdout) == ["[]", "[]"], out.stdout
