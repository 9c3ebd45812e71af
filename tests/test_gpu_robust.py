"""GPU parity of the robust-score kernels (``k_robust_cols`` in both its forms, ``k_robust_rank``) and of the robust step of
a report against the NumPy restatement of tests/robust_oracle_backend.py.  Every column and every rank of every case is
compared.

Bounds: column records, section ratios and section z bit for bit (an actual value; two f32 products and a maximum; one f64
quotient rounded to f32); NaN and inf masks equal; GPU slots within 2e-6 * max(1, |expected|), the tolerance
tests/test_gpu_tail.py uses for the same f64 weighted mean summed in another order."""
import ctypes

import numpy as np
import pytest
import torch

import robust_workers
from mp_util import run_ranks
from followup_cases import ROBUST_SHAPES
from robust_oracle_backend import robust_scores_table
from score_cases import case_table
from test_gpu_score import _random_table

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3, 0), (2, 2, 2), (3, 5, 6), (4, 0, 7), (5, 4, 4), (63, 17, 33), (64, 17, 33), (65, 0, 64), (100, 7, 9),
          (4096, 32, 16), (8, 4096, 8)] + list(ROBUST_SHAPES)  # (the boundaries of k_robust_cols: tests/followup_cases.py)
SPECIALS = ("full", "single", "equal", "zero_inf", "repeated", "mostly_inf")
ALL_BUT_FAST = [0, 1, 2, 3, 4, 6, 7]


@pytest.fixture(scope="module")
def be():
    from nvrx_straggler.backend import get_backend

    return get_backend()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _special(T, rng, c, kind, K, S):
    """Rewrite column ``c`` of the table's med part (and, for a kernel column, its weights) as one of the issue's columns."""
    R, KS = T.shape[0], K + S
    col = np.full(R, -1.0, dtype=np.float32)
    if kind == "full":  # a column nobody misses
        col[:] = rng.lognormal(1.0, 0.5, R)
    elif kind == "single":  # present on a single rank
        col[rng.integers(R)] = np.float32(rng.lognormal(1.0, 0.5))
    elif kind == "equal":  # mad = 0: the floor decides
        col[:] = np.float32(3.25)
    elif kind == "zero_inf":  # a 0.0 and a +inf among ordinary values
        col[:] = rng.lognormal(1.0, 0.5, R)
        col[rng.random(R) < 0.15] = -1.0
        col[0] = 0.0
        col[R - 1] = np.inf if R > 1 else 0.0
    elif kind == "repeated":  # repeated values across the median position
        col[:] = rng.lognormal(1.0, 0.5, R)
        order = np.argsort(col, kind="stable")
        mid = (R - 1) >> 1
        col[order[max(0, mid - 2) : mid + 3]] = col[order[mid]]
    elif kind == "mostly_inf":  # more than half the ranks hold +inf: ctr = inf, the deviations inf - inf = NaN and
        col[:] = rng.lognormal(1.0, 0.5, R)  # |finite - inf| = inf; a NaN deviation orders above +inf, so mad = NaN
        col[rng.permutation(R)[: R // 2 + 1]] = np.inf
    T[:, c] = col
    if c < K:
        T[:, 2 * KS + c] = np.where(col >= 0, rng.uniform(1, 1000, R), 0.0).astype(np.float32)


def _tables(R, K, S):
    """The tables of one case: ``_random_table`` with 15 % of the medians absent plus the six special columns, spread over
    the columns (a case with fewer than six columns gets several tables, so that each special column is exercised), each
    with the columns whose records hold NaN of the arithmetic's own making (``mostly_inf``)."""
    rng = np.random.default_rng(R * 1000 + K + S)
    KS = K + S
    todo = list(SPECIALS)
    while todo:
        T = _random_table(rng, R, K, S)
        take, todo = todo[:KS], todo[KS:]
        cols = np.linspace(0, KS - 1, len(take)).astype(int) if len(take) > 1 else [KS // 2]
        for c, kind in zip(cols, take):
            _special(T, rng, int(c), kind, K, S)
        yield T, [int(c) for c, kind in zip(cols, take) if kind == "mostly_inf"]


def _run(be, T, K, S, first_rank, n_ranks, min_ranks, floor_rel):
    R = T.shape[0]
    ws = be.workspace(R, K, S, R, 0)
    ws.robust_settle()
    ws.send.copy_(torch.from_numpy(T))
    torch.cuda.synchronize()
    return be.robust_score(ws, ws.send, first_rank, n_ranks, min_ranks, floor_rel).records()


def _compare(got, exp, tag, nan_cols=()):
    """``nan_cols``: columns whose mad / scale are NaN by arithmetic (inf - inf, 0 * inf), not the "no reference" NaN the
    kernel writes itself: their float words are compared by NaN-ness, a NaN's sign and payload being nobody's contract.
    Every other word of every record is compared bit for bit."""
    (gcols, gsc), (ecols, esc) = got, exp
    assert gcols.shape == ecols.shape and gsc.shape == esc.shape, tag
    differ = gcols != ecols
    for c in nan_cols:
        gf, ef = gcols[c, :3].view(np.float32), ecols[c, :3].view(np.float32)
        assert np.array_equal(np.isnan(gf), np.isnan(ef)), (tag, "column", c, gf, ef)
        differ[c, :3] &= ~np.isnan(ef)
    bad = np.flatnonzero(differ.any(axis=1))
    assert bad.size == 0, (tag, "columns", bad[:8].tolist(), gcols[bad[:4]], ecols[bad[:4]],
                           gcols[bad[:4]].view(np.float32), ecols[bad[:4]].view(np.float32))
    assert np.array_equal(np.isnan(gsc), np.isnan(esc)), (tag, "NaN masks", np.argwhere(np.isnan(gsc) != np.isnan(esc))[:8])
    assert np.array_equal(np.isposinf(gsc), np.isposinf(esc)) and np.array_equal(np.isneginf(gsc), np.isneginf(esc)), (tag, "inf masks")
    sec_g, sec_e = gsc[:, :, 1:], esc[:, :, 1:]
    ok = ~np.isnan(sec_e)
    bad = np.argwhere(ok & (_bits(sec_g) != _bits(sec_e)))
    assert bad.size == 0, (tag, "sections", bad[:8].tolist(), sec_g[tuple(bad[:8].T)], sec_e[tuple(bad[:8].T)])
    g, e = gsc[:, :, 0].astype(np.float64), esc[:, :, 0].astype(np.float64)
    fin = np.isfinite(e)
    if fin.any():
        err = np.abs(g[fin] - e[fin]) / np.maximum(1.0, np.abs(e[fin]))
        print(tag, "GPU slots: max error", float(err.max()), "of", int(fin.sum()))
        assert err.max() <= 2e-6, (tag, "GPU slots", float(err.max()))


@pytest.mark.parametrize("R,K,S", SHAPES)
def test_robust_score_matches_numpy(be, R, K, S):
    for t, (T, nan_cols) in enumerate(_tables(R, K, S)):
        for min_ranks in (1, 4):
            for floor_rel in (0.0, 0.02):
                tag = (R, K, S, t, min_ranks, floor_rel)
                got = _run(be, T, K, S, 0, R, min_ranks, floor_rel)
                exp = robust_scores_table(T, K, S, 0, R, min_ranks, floor_rel)
                _compare(got, exp, tag, nan_cols)
                for c in nan_cols:
                    ctr, mad, _, n = exp[0][c]
                    if n >= min_ranks:  # what the header defines for this column
                        assert ctr == 0x7F800000 and np.isnan(np.uint32(mad).view(np.float32)), (tag, exp[0][c])
                if min_ranks == 4 and floor_rel == 0.02:
                    # a sub-range of ranks equals the slice of the full result, bit for bit
                    lo, n = (R // 3, max(1, R // 2)) if R > 1 else (0, 1)
                    pcols, psc = _run(be, T, K, S, lo, n, min_ranks, floor_rel)
                    assert np.array_equal(pcols, got[0]) and np.array_equal(_bits(psc), _bits(got[1][lo : lo + n])), tag


@pytest.mark.parametrize("R,K,S", [(2, 2, 2), (5, 8, 8), (64, 12, 3), (65, 12, 3), (100, 7, 9), (1025, 2, 2)])
def test_robust_score_on_edge_tables(be, R, K, S):
    """``score_cases.case_table("edge_common")``: NaN medians (absent by ``v >= 0``), a column of -1 only and a one-rank column
    under both ``min_ranks``, zero and infinite medians, thirty orders of magnitude inside one column, a rank whose weights
    are all zero."""
    T = case_table("edge_common", R, K, S)
    for min_ranks in (1, 4):
        for floor_rel in (0.0, 0.02):
            tag = ("edge_common", R, K, S, min_ranks, floor_rel)
            got = _run(be, T, K, S, 0, R, min_ranks, floor_rel)
            _compare(got, robust_scores_table(T, K, S, 0, R, min_ranks, floor_rel), tag)
    lo, n = R // 3, max(1, R // 2)
    pcols, psc = _run(be, T, K, S, lo, n, 4, 0.02)
    assert np.array_equal(pcols, got[0]) and np.array_equal(_bits(psc), _bits(got[1][lo : lo + n]))


def test_argument_errors_come_back_before_the_device_is_touched(be):
    from nvrx_straggler import _native

    lib = be.lib
    R, K, S = 8, 8, 2
    table = torch.zeros((R, _native.table_len(K, S)), dtype=torch.float32, device="cuda")
    out = torch.full((_native.robust_words(R, K, S),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def score(tp=table.data_ptr(), R=R, first=0, n=R, min_ranks=4, floor=0.02, op=out.data_ptr()):
        return lib.nvrx_robust_score(tp, R, K, S, first, n, min_ranks, floor, op, be._stream_handle)

    assert score(tp=None) == _native.ERR_INVALID and score(op=None) == _native.ERR_INVALID
    assert score(R=_native.ROBUST_MAX_RANKS + 1, n=1) == _native.ERR_RANGE
    assert score(first=7, n=2) == _native.ERR_RANGE and score(first=-1) == _native.ERR_RANGE and score(n=R + 1) == _native.ERR_RANGE
    assert score(min_ranks=0) == _native.ERR_RANGE
    assert score(floor=float("nan")) == _native.ERR_INVALID
    assert score(op=out.data_ptr() + 4) == _native.ERR_INVALID
    desc = _native.ReportDesc()
    desc.R, desc.K, desc.S = R, K, S
    assert lib.nvrx_report_robust(None, ctypes.byref(desc), 0, R, 4, 0.02, out.data_ptr()) == _native.ERR_INVALID
    be.synchronize()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x5A5A5A5A).all()  # nothing was launched


# ---- the robust step of a report ------------------------------------------------------------------------------------------
_NAMES = [f"section_{s:03d}" for s in range(64)]


def _check_scenario(rep, explained=()):
    assert rep["median_flagged"] == ALL_BUT_FAST, rep["median_flagged"]
    assert rep["robust_flagged"] == [robust_workers.SLOW_RANK], rep["robust_flagged"]
    assert rep["explained"] == list(explained)
    med = robust_workers.scenario_medians()
    t = rep["robust"]
    assert t["min_ranks"] == 4 and t["floor"] == 0.02 and sorted(t["gpu_z"]) == list(range(8))
    for s, n in enumerate(_NAMES):
        ctr = np.sort(med[:, s])[3]  # NumPy's lower median of the eight medians
        assert t["section_center"][n] == float(ctr), (n, t["section_center"][n], float(ctr))
        assert t["ranks_with_data"][n] == 8
        for r in range(8):
            assert t["section_ratio"][n][r] == float(np.float32(np.float64(ctr) / np.float64(med[r, s]))), (n, r)


def test_scenario_folded_in_one_process(be):
    samples = robust_workers.scenario_samples()
    assert np.array_equal(np.sort(samples, axis=2)[:, :, 16], robust_workers.scenario_medians())
    out = robust_workers.folded_scenario(0, 1)
    assert len(out) == 3
    for rep in out:
        _check_scenario(rep)


def test_scenario_on_four_processes_sharing_the_gpu_with_attribution():
    """Default route (gloo / c10d), kernel attribution on as well: both follow-up launches behind one report, both read later."""
    res = run_ranks(robust_workers.folded_scenario, 4, timeout=420, use_oracle_backend=False, device=0, kernel_attribution=3)
    assert all(r == [None] * 3 for r in res[1:])
    for rep in res[0]:
        _check_scenario(rep, explained=("relative",))


def test_asynchronous_reports_copy_out_once_and_match_their_own_window():
    res = run_ranks(robust_workers.ring_windows_asynchronous, 1, timeout=300, use_oracle_backend=False, device=0)[0]
    samples, names = res["samples"], res["names"]
    assert res["enqueue_only"] and len(res["reports"]) == samples.shape[0] == 40
    k = (samples.shape[2] - 1) >> 1
    for w, rep in enumerate(res["reports"]):
        t = rep["robust"]
        exp = np.sort(samples[w], axis=1)[:, k]
        got = np.array([t["section_center"][n] for n in names], dtype=np.float32)
        assert np.array_equal(_bits(got), _bits(exp)), (w, got, exp)
        assert all(v == {0: 1.0} for v in t["section_ratio"].values()) and all(v == {0: 0.0} for v in t["section_z"].values())
        assert t["min_ranks"] == 1 and all(v == 1 for v in t["ranks_with_data"].values())
        at_return, before, after_first, after_second = rep["copy_outs"]
        # neither the report call nor scores / stragglers copy robust scores out; the first robust_scores() does, exactly once
        assert at_return == before == w and after_first == after_second == w + 1, (w, rep["copy_outs"])


def test_detector_in_stamp_mode_one_process():
    res = run_ranks(robust_workers.detector_one_process, 1, timeout=300, use_oracle_backend=False, device=0,
                    env={"NVRX_GPU_TIMING": "stamp"})[0]
    assert res["on"] and res["lane_is_none"]
    for w in res["windows"]:
        t = w["robust"]
        assert t["gpu_z"] == {0: 0.0} and t["gpu_ratio"] == {0: 1.0} and w["flagged"] == []
        assert "work" in t["section_z"] and all(v == {0: 0.0} for v in t["section_z"].values()) and t["min_ranks"] == 1
        assert any(k.startswith("hipevent::work") for k in t["kernel_center"])
