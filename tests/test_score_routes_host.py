"""The score dispatch without a GPU: ``nvrx_score_route`` (the function ``nvrx_score`` and the one-call report switch on)
against the shapes of tests/score_cases.py, the routes of every shape the GPU suite scores, and the C oracle on the edge
tables the GPU test compares the kernels with."""
import numpy as np
import pytest

import score_cases as sc
from oracle import oracle
from score_cases import ROWS, ROWS_PRE, SINGLE, TILE8, TILE16

ALIGNED = 0x7F0000001000  # any 16-byte aligned address: the function looks at the low bits only


@pytest.fixture(scope="module")
def route():
    from nvrx_straggler import _native

    lib = _native.load()  # loads without a GPU
    assert (_native.ROUTE_SINGLE, _native.ROUTE_ROWS, _native.ROUTE_ROWS_PRE, _native.ROUTE_TILE16, _native.ROUTE_TILE8) == \
        (SINGLE, ROWS, ROWS_PRE, TILE16, TILE8)

    def f(R, K, S, d_scores=ALIGNED, d_flags=ALIGNED):
        return lib.nvrx_score_route(R, K, S, d_scores, d_flags)

    return f


def test_header_and_binding_declare_the_route_query():
    import os
    import re

    from nvrx_straggler import _native

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nvrx_straggler.h")).read()
    got = dict(re.findall(r"^#define NVRX_SCORE_ROUTE_(\w+) (\d+)$", header, flags=re.M))
    assert {k: int(v) for k, v in got.items()} == {"SINGLE": SINGLE, "ROWS": ROWS, "ROWS_PRE": ROWS_PRE, "TILE16": TILE16, "TILE8": TILE8}
    assert "nvrx_score_route" in {name for name, _, _ in _native.SYMBOLS}
    assert re.search(r"^#define NVRX_ABI_VERSION 2$", header, flags=re.M)


def test_every_listed_shape_takes_the_listed_route(route):
    for (R, K, S), exp in sc.ROUTE_SHAPES.items():
        assert route(R, K, S) == exp, ((R, K, S), sc.ROUTE_NAMES[exp])
    assert set(sc.ROUTE_SHAPES.values()) == {SINGLE, ROWS, ROWS_PRE, TILE16, TILE8}


def test_the_boundaries_are_where_the_lds_budgets_put_them(route):
    """Both sides of every threshold, from the arithmetic of the header's comment (no shape list involved)."""
    def single_bytes(R, K, S):
        nout = R * (2 + 2 * S)
        return ((K + S + 3) & ~3) * 4 + ((nout + 3) & ~3) * 4 + ((nout + 15) & ~15)

    def tile_bytes(t, S):
        nout = t * (2 + 2 * S)
        return ((nout + 3) & ~3) * 4 + ((nout + 15) & ~15)

    for R in (1, 2, 7, 8, 16, 33, 61, 64):
        for K in (0, 5, 4096, 12248, 13000):
            for S in (0, 1, 40, 94, 95, 191, 192, 767, 768, 12288 - K if K < 12288 else 0, 12289 - K if K < 12289 else 1):
                exp = SINGLE if single_bytes(R, K, S) <= 60 * 1024 else ROWS if (K + S) * 4 <= 48 * 1024 else ROWS_PRE
                assert route(R, K, S) == exp, (R, K, S)
    for R in (65, 70, 100, 1024, 4096):
        for K in (0, 3, 13000):
            for S in (0, 9, 64, 306, 307, 613, 614, 5000):
                exp = TILE16 if tile_bytes(16, S) <= 48 * 1024 else TILE8 if tile_bytes(8, S) <= 48 * 1024 else ROWS_PRE
                assert route(R, K, S) == exp, (R, K, S)
    assert tile_bytes(16, 306) <= 48 * 1024 < tile_bytes(16, 307) and tile_bytes(8, 613) == 49120 and tile_bytes(8, 614) > 48 * 1024
    assert single_bytes(16, 13000, 40) == 58720


def test_unaligned_result_arrays_leave_the_sixteen_byte_routes(route):
    for (R, K, S), exp in sc.ROUTE_SHAPES.items():
        for off_s, off_f in ((4, 0), (0, 1), (8, 8), (0, 15)):
            got = route(R, K, S, ALIGNED + off_s, ALIGNED + off_f)
            if exp == SINGLE:  # one workgroup per rank; column minima beyond 48 KB of LDS get their own pass
                assert got == (ROWS if (K + S) * 4 <= 48 * 1024 else ROWS_PRE), (R, K, S)
            elif exp in (TILE16, TILE8):
                assert got == ROWS_PRE, (R, K, S)
            else:
                assert got == exp, (R, K, S)
    assert route(64, 0, 94, ALIGNED + 4) == ROWS and route(16, 13000, 40, ALIGNED, ALIGNED + 1) == ROWS_PRE


def test_bad_shapes_are_an_error(route):
    from nvrx_straggler import _native

    for R, K, S in ((0, 1, 1), (-1, 0, 0), (1, -1, 0), (1, 0, -1), (-5, -5, -5)):
        assert route(R, K, S) == _native.ERR_INVALID
    assert b"bad table shape" in _native.load().nvrx_last_error()
    assert route(1, 0, 0) == SINGLE and route(65, 0, 0) == TILE16


# Every (R, K, S) a tests/test_gpu_*.py scores, with the route its (aligned) workspace takes: what the suite covers.
# test_gpu_score_routes.py asserts the routes of sc.ROUTE_SHAPES on the GPU; the other files' shapes are listed here.
GPU_SUITE_SHAPES = {
    # test_gpu_score.py: test_score_kernel_matches_oracle, test_completion_word_never_precedes_the_results
    (1, 0, 1): SINGLE, (1, 3, 0): SINGLE, (2, 2, 2): SINGLE, (8, 0, 64): SINGLE, (8, 5, 6): SINGLE, (8, 4096, 8): SINGLE,
    (64, 17, 33): SINGLE, (100, 7, 9): TILE16, (3, 0, 0): SINGLE, (16, 13000, 40): SINGLE, (65, 0, 64): TILE16,
    (1024, 0, 64): TILE16, (4096, 32, 16): TILE16, (8, 5, 64): SINGLE, (64, 0, 64): SINGLE,
    # test_gpu_attribution.py / test_gpu_tail.py / test_gpu_onset.py / test_gpu_period.py: subsets of the above
    # test_gpu_robust.py
    (3, 5, 6): SINGLE, (4, 0, 7): SINGLE, (5, 4, 4): SINGLE, (63, 17, 33): SINGLE,
    # test_gpu_detector.py: test_one_call_report_beyond_the_single_workgroup_scorer (R folded ranks x 8 sections)
    (65, 0, 8): TILE16, (96, 0, 8): TILE16, (512, 0, 8): TILE16,
    # test_gpu_score_routes.py: the one-call report on ROWS, scratch regrowth
    (64, 0, 96): ROWS, (1024, 100, 64): TILE16,
    **sc.ROUTE_SHAPES,
}


def test_routes_of_every_shape_the_gpu_suite_scores(route):
    for (R, K, S), exp in GPU_SUITE_SHAPES.items():
        assert route(R, K, S) == exp, ((R, K, S), sc.ROUTE_NAMES[exp])
    assert set(GPU_SUITE_SHAPES.values()) == {SINGLE, ROWS, ROWS_PRE, TILE16, TILE8}


@pytest.mark.parametrize("R,K,S", list(sc.ROUTE_SHAPES) + [sc.REGROW_SHAPES[1]])
def test_oracle_on_the_edge_tables(R, K, S):
    """The oracle alone: NaN, inf and 0 appear where ``edge_table`` planted them, and no GPU score of any table the GPU
    test scores lies within ``4e-6 * threshold`` of its threshold -- the condition under which that test may demand every
    flag (a GPU score is 2e-6 from the oracle's at most)."""
    for kind in sc.TABLE_KINDS:
        T = sc.case_table(kind, R, K, S)
        assert not np.signbit(T[T == 0]).any()  # no -0.0
        for do_indiv, do_rel in sc.COMBOS:
            exp = oracle.score_table(T, K, S, do_indiv, do_rel)
            assert sc.gpu_scores_near_threshold(exp, S) == 0, (kind, do_indiv, do_rel)
            fin = exp[np.isfinite(exp) & (exp != 0)]
            assert fin.size == 0 or np.abs(fin).min() >= np.finfo(np.float32).tiny  # no subnormal quotient
    for kind in ("edge", "edge_common"):
        T = sc.case_table(kind, R, K, S)
        plan = sc.edge_plan(R, K, S, lacking_rank=(kind == "edge"))
        exp = oracle.score_table(T, K, S, True, True)
        fl = sc.expected_flags(exp, S)
        ind, rel = exp[:, 2 : 2 + S], exp[:, 2 + S :]
        find, frel = fl[:, 2 : 2 + S], fl[:, 2 + S :]
        assert int(T[:, -1].sum()) == R - 1 and T[R - 1, -1] == 0
        p = plan["section"]
        if S >= 8:
            assert set(p) == set(sc.COLUMN_KINDS)
        if K + S >= 8:
            assert set(p) | set(plan["kernel"]) == set(sc.COLUMN_KINDS)
        if "zero_zero" in p:
            c, r = p["zero_zero"]
            assert np.isnan(ind[r, c]) and np.isnan(rel[r, c]) and not find[r, c] and not frel[r, c]
        if "zero_pos" in p:
            c, r = p["zero_pos"]
            assert ind[r, c] == np.inf and not find[r, c] and np.isnan(rel[r, c])
            others = (T[:, K + c] > 0)
            assert (rel[others, c] == 0).all() and frel[others, c].all()  # a zero minimum: everybody else scores 0
        if "inf" in p:
            c, r = p["inf"]
            assert ind[r, c] == 0 and find[r, c]
            if R >= 2:
                assert rel[r, c] == 0 and frel[r, c]
        if "nan" in p:
            c, r = p["nan"]
            assert np.isnan(ind[r, c]) and np.isnan(rel[r, c])
            if R >= 2 and (T[:, K + c] >= 0).any():
                assert np.isfinite(rel[T[:, K + c] >= 0, c]).all()  # ... and the NaN did not reach the column minimum
        if "nobody" in p:
            c, _ = p["nobody"]
            assert np.isnan(ind[:, c]).all() and np.isnan(rel[:, c]).all()
        if "one_rank" in p:
            c, r = p["one_rank"]
            assert ind[r, c] == 0.75 == sc.THRESHOLDS[3] and not find[r, c] and np.isnan(np.delete(ind[:, c], r)).all()
            assert np.isnan(rel[:, c]).all() if R >= 2 else rel[r, c] == 1  # (the -1 of the others wins the minimum)
        if "equal" in p:
            c, r = p["equal"]
            assert (np.delete(rel[:, c], r) == 1).all()
            if R >= 2:
                assert rel[r, c] == 0.5 == sc.THRESHOLDS[1] and not frel[r, c]  # on the threshold: strict compare, no flag
        if "wide" in p:
            c, r = p["wide"]
            assert rel[r, c] == 1
            if R >= 2:
                q = np.float32(np.float64(np.float32(1e-15)) / np.float64(np.float32(1e15)))
                assert (np.delete(rel[:, c], r) == q).all() and 0.9e-30 < q < 1.1e-30
        if plan["zero_w"] is not None:
            r = plan["zero_w"]
            assert (T[r, :K] >= 0).any()  # it has kernels ...
            assert np.isnan(exp[r, 0]) and not fl[r, 0]  # ... and 0/0 for a score
        if plan["lack"] is not None:
            assert np.isnan(exp[:, 1]).all() and np.isnan(exp[plan["lack"], 0])
        elif K > 0 and R >= 3:  # (of two ranks one weighs nothing and the other divides 0 by 0)
            assert np.isfinite(exp[:, 1]).any()  # without the lacking rank the relative GPU scores are there to compare
        pk = plan["kernel"]
        if "zero_pos" in pk:
            c, r = pk["zero_pos"]
            if r != plan["zero_w"] and pk.get("zero_zero", (None, None))[1] != r:
                assert exp[r, 0] == np.inf and not fl[r, 0]
