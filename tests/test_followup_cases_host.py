"""The conditions that keep the follow-up parity tests on the GPU (tests/test_gpu_followup_parity.py) from passing vacuously,
asserted on the builders of tests/followup_cases.py and on the NumPy formulas alone: the relative references are alive,
every reported rank has kernels and sections to compare, and every planted value reaches the formula.

The liveness conditions hold for the "live" and "edge_common" tables.  An "edge" table keeps ``score_cases``' rank that lacks
every kernel: there the relative family of EVERY rank has no eligible kernel, which is that case's point, and it is asserted
as such; its individual family is held to the same conditions."""
import numpy as np
import pytest

from attribution_oracle_backend import attribute_table, column_minima, loss_terms, rank_by_loss
from followup_cases import (FOLLOWUP_SHAPES, PLANE_KINDS, TABLE_KINDS, attribution_extras, dead_by_plan, extras_plan,
                            family_scores_table, followup_planes, followup_table, live_columns, live_table, plane_plan, tie_ids)
from nvrx_straggler.row_families import FAMILIES
from score_cases import edge_plan


def _bits64(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _special_ranks(kind, R, K, S):
    """The ranks the liveness conditions leave out: ``edge_plan``'s kernel-less and zero-weight ranks."""
    if kind == "live":
        return set()
    ep = edge_plan(R, K, S, lacking_rank=(kind == "edge"))
    return {ep["lack"], ep["zero_w"]} - {None}


def test_ordering_contract_of_rank_by_loss():
    """Descending by value; -0.0 and +0.0 tie; NaN after -inf whatever its sign bit; ties to the lower id."""
    neg_nan = np.array([0xFFF8000000000000], dtype=np.uint64).view(np.float64)[0]
    pos_nan = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]
    assert np.signbit(neg_nan) and not np.signbit(pos_nan)
    ids = np.array([3, 4, 5, 6, 7, 8, 9, 10, 11, 12])
    lost = np.array([0.0, -0.0, pos_nan, np.inf, 2.5, -np.inf, neg_nan, 2.5, -0.0, -1.0])
    assert ids[rank_by_loss(ids, lost)].tolist() == [6, 7, 10, 3, 4, 11, 12, 8, 5, 9]
    # the same values under other ids: the order of the ties follows the ids, not the bit patterns
    ids2 = ids[::-1].copy()
    # (-0.0 at id 4 before +0.0 at id 12; the NaN with the sign bit set, id 6, before the one without)
    assert ids2[rank_by_loss(ids2, lost)].tolist() == [9, 5, 8, 4, 11, 12, 3, 7, 6, 10]


@pytest.mark.parametrize("R,K,S", FOLLOWUP_SHAPES)
@pytest.mark.parametrize("kind", TABLE_KINDS)
def test_tables_keep_their_references_alive(kind, R, K, S):
    T = followup_table(kind, R, K, S)
    KS = K + S
    assert T.shape[0] == R and T.dtype == np.float32
    if K < 2 or R < 2:
        return
    ep = edge_plan(R, K, S, lacking_rank=(kind == "edge")) if kind != "live" else {"kernel": {}, "section": {}}
    special = _special_ranks(kind, R, K, S)
    others = [r for r in range(R) if r not in special]
    if kind == "edge":
        # the kernel-less rank: no kernel column has a reference, by design
        assert np.isnan(column_minima(T[:, :K])).all()
        rows = T[[r for r in range(R) if r != ep["lack"]]]
    else:
        rows = T
    alive, counted = live_columns(rows[:, :K], dead_by_plan(ep, "kernel"))
    assert alive >= max(1, counted // 2), (alive, counted)
    for r in others:
        for fam in (0, 1):
            ids = loss_terms(T, K, S, r, fam)[0]
            if fam == 1 and kind == "edge":
                assert ids.size == 0
            else:
                assert ids.size >= 2, (r, fam, ids)


@pytest.mark.parametrize("R,K,S", [s for s in FOLLOWUP_SHAPES if s[0] >= 64])
def test_per_entry_absences_would_leave_no_reference(R, K, S):
    """What the older parity tests build: 15 % of the entries absent independently.  From 64 ranks on no column survives."""
    rng = np.random.default_rng([R, K, S])
    T = live_table(rng, R, K, S, p_holes=1.0)
    assert live_columns(T[:, : K + S])[0] == 0
    assert all(loss_terms(T, K, S, r, 1)[0].size == 0 for r in range(0, R, 7))


@pytest.mark.parametrize("R,K,S", FOLLOWUP_SHAPES)
@pytest.mark.parametrize("kind", PLANE_KINDS)
@pytest.mark.parametrize("fam", FAMILIES, ids=lambda f: f.name)
def test_planes_keep_their_references_alive(fam, kind, R, K, S):
    planes, T = followup_planes(kind, fam, R, K, S)
    KS = K + S
    assert planes.shape == (R, fam.planes, KS) and planes.dtype == np.float32
    v = planes[:, 0, :]
    with np.errstate(invalid="ignore"):
        have = ~(v < 0)
        # no other plane holds a value of plane 0, and every plane is absent where plane 0 is
        assert (planes[:, 1:, :][np.broadcast_to(have[:, None, :], planes[:, 1:, :].shape)] >= 100.0).all()
        assert (planes[:, 1:, :][np.broadcast_to(~have[:, None, :], planes[:, 1:, :].shape)] == -1.0).all()
        assert not (v[have & np.isfinite(v)] >= 100.0).any() or kind == "edge"  # ("wide" holds 1e15)
    if R < 2:
        return
    plan = plane_plan(R, K, S) if kind == "edge" else {"kernel": {}, "section": {}}
    exp = family_scores_table(fam, planes, T, K, S)
    # a NaN GPU slot: the two ranks whose weights are all zero (W = 0), and the rank of the kernel column's 0/0
    zero_w = {edge_plan(R, K, S)["zero_w"], edge_plan(R, K, S)["lack"]} - {None} if kind == "edge" else set()
    if "zero_zero" in plan["kernel"]:
        zero_w.add(plan["kernel"]["zero_zero"][1])
    if K >= 2:
        alive, counted = live_columns(v[:, :K], dead_by_plan(plan, "kernel"))
        assert alive >= max(1, counted // 2), (alive, counted)
        ref = column_minima(v[:, :K])
        for r in range(R):
            with np.errstate(invalid="ignore"):
                elig = int(((v[r, :K] >= 0) & ~np.isnan(ref)).sum())
            assert elig >= 2, (r, elig)
            assert np.isnan(exp[r, 0]) == (r in zero_w), (r, exp[r, 0])
    if S >= 2:
        alive, counted = live_columns(v[:, K:], dead_by_plan(plan, "section"))
        assert alive >= max(1, counted // 2), (alive, counted)
        assert ((~np.isnan(exp[:, 1:])).sum(axis=1) >= 2).all()
    if kind == "edge":
        sec = plan["section"]
        for what, (c, r) in sec.items():
            col = exp[:, 1 + c]
            rest = np.arange(R) != r
            if what == "zero_zero":
                assert np.isnan(col[r]) and (col[rest] == 0.0).all()  # 0/0, and 0 / v
            elif what == "inf":
                assert col[r] == 0.0 and (col[rest] > 0).all()
            elif what == "nan":
                assert np.isnan(col[r]) and not np.isnan(col[rest]).any()
            elif what in ("nobody", "one_rank"):
                assert np.isnan(col).all()
            elif what == "equal":
                assert col[r] == 0.5 and (col[rest] == 1.0).all()
            elif what == "wide":
                assert col[r] == 1.0 and (col[rest] == np.float32(1e-30)).all()
        if K > 0:
            assert edge_plan(R, K, S)["zero_w"] is not None and (T[edge_plan(R, K, S)["zero_w"], 2 * KS : 2 * KS + K] == 0).all()


@pytest.mark.parametrize("R,K,S", [s for s in FOLLOWUP_SHAPES if extras_plan(s[0], s[1]) is not None])
@pytest.mark.parametrize("kind", TABLE_KINDS)
def test_every_planted_value_reaches_the_formula(kind, R, K, S):
    T = followup_table(kind, R, K, S)
    plan = extras_plan(R, K)
    r, t = plan["rank"], plan["tie_rank"]
    ids, s, n, w = loss_terms(T, K, S, r, 0)
    at = {int(k): i for i, k in enumerate(ids)}
    i_inf, i_z0, i_zp, i_m0, i_p0, i_ni = (at[plan[key]] for key in ("zero_times_minus_inf", "zero_w_zero_zero",
                                                                     "pos_w_zero_zero", "minus_zero", "plus_zero", "minus_inf"))
    # the three sources of a NaN lost_us, and a score of +inf
    assert s[i_inf] == np.inf and np.isnan(n[i_inf]) and w[i_inf] == 0
    assert np.isnan(s[i_z0]) and np.isnan(n[i_z0]) and w[i_z0] == 0
    assert np.isnan(s[i_zp]) and np.isnan(n[i_zp]) and w[i_zp] > 0
    assert s[i_ni] == np.inf and n[i_ni] == -np.inf  # a -inf lost_us
    # -0.0 at the lower id, +0.0 at the higher one: they tie by value
    assert _bits64(n[i_m0]) == 0x8000000000000000 and _bits64(n[i_p0]) == 0 and ids[i_m0] < ids[i_p0]
    order = ids[rank_by_loss(ids, n)].tolist()
    assert order.index(plan["minus_zero"]) + 1 == order.index(plan["plus_zero"])
    # every NaN after every -inf, each group in id order (score_cases' own plants may add to either on this rank)
    nans, neg = ids[np.isnan(n)].tolist(), ids[np.isneginf(n)].tolist()
    assert order[-len(nans) :] == nans and order[-len(nans) - len(neg) : -len(nans)] == neg
    assert {plan["zero_times_minus_inf"], plan["zero_w_zero_zero"], plan["pos_w_zero_zero"]} <= set(nans) and plan["minus_inf"] in neg
    exp = attribute_table(T, K, S, 16, True, True)
    f32, i32 = exp.view(np.float32), exp.view(np.int32)
    if K == 16:
        # every eligible kernel of the rank is listed: the NaN come last, the zeros in id order and both as +0.0
        listed = i32[r, 0, 1:, 0].tolist()
        assert listed[: ids.size] == order and listed[ids.size :] == [-1] * (16 - ids.size)
        lost = f32[r, 0, 1 : 1 + ids.size, 3]
        assert np.isnan(lost[-3:]).all()
        j = listed.index(plan["minus_zero"])
        assert exp[r, 0, 1 + j, 3] == 0 and exp[r, 0, 2 + j, 3] == 0 and listed[j + 1] == plan["plus_zero"]
    # a zero-weight kernel with a zero median whose column the others have: 0 * (1 - 0 / 0) in the relative family too
    if kind != "edge":
        ids1, s1, n1, _ = loss_terms(T, K, S, r, 1)
        assert plan["zero_w_zero_zero"] in ids1 and np.isnan(n1[list(ids1).index(plan["zero_w_zero_zero"])])
    assert np.isneginf(f32[r, 0, 0, 0]) or np.isnan(f32[r, 0, 0, 0])  # the rank's whole deficit: -inf + NaN
    # a header with W = 0 although the rank has kernels: listed, with 0/0 shares
    z = plan["zero_w"]
    assert f32[z, 0, 0, 3] == 0.0 and exp[z, 0, 0, 2] > 0 and np.isnan(f32[z, 0, 0, 0])
    assert np.isnan(f32[z, 0, 1, 1]) and i32[z, 0, 1, 0] >= 0
    # the tie run: identical terms, above everything else on its rank, in both families where the relative one lives
    tie = list(plan["tie"])
    assert tie == list(tie_ids(K)) and len(tie) >= (20 if K >= 34 else K - 14) and min(tie) >= 14
    if K >= 255:  # neighbours, lanes of four waves
        assert {14, 15, 78, 142, 206} <= set(tie)
    if K >= 1024:  # one thread's four strides of k_attribute<256>
        assert {14, 270, 526, 782} <= set(tie)
    if K in (257, 1025):  # the one id of the last stride
        assert K - 1 in tie
    for fam in ((0,) if kind == "edge" else (0, 1)):
        idt, _, nt, _ = loss_terms(T, K, S, t, fam)
        in_run = np.isin(idt, tie)
        assert in_run.sum() == len(tie) and (nt[in_run] == 3072.0).all()
        with np.errstate(invalid="ignore"):
            assert not (nt[~in_run] >= 3072.0).any()
        shown = min(16, len(tie))
        assert i32[t, fam, 1 : 1 + shown, 0].tolist() == tie[:shown]  # the lowest ids of the run, in id order
        if len(tie) >= 16:
            assert (f32[t, fam, 1:, 3] == 3072.0).all()  # a tie run that fills all 16 entries


def test_extras_leave_small_tables_alone():
    for R, K in ((2, 40), (5, 15)):
        T = followup_table("live", R, K, 2)
        assert extras_plan(R, K) is None and np.array_equal(attribution_extras(T.copy(), R, K, 2), T, equal_nan=True)
