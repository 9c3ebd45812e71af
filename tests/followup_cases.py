"""Shared inputs of the follow-up scorer tests (tests/test_followup_cases_host.py on the CPU, tests/test_gpu_followup_parity.py
and tests/test_gpu_robust.py on the GPU): the kernels that read the exchanged table after the main scorer -- ``k_attribute``,
``k_tail_score`` behind the four row families, ``k_robust_cols`` / ``k_robust_rank`` and the column minima on their call
paths.  Tables and planes whose relative references are ALIVE (absences drawn per column, as ``score_cases.edge_table``
draws them), the edge values of ``score_cases``, NaN / signed-zero / tied ``n_k`` for the ordering of ``k_attribute``, and
the smallest shapes on both sides of every boundary these paths have."""
import numpy as np

from episode_oracle_backend import episode_scores_table
from onset_oracle_backend import onset_scores_table
from period_oracle_backend import period_scores_table
from score_cases import COLUMN_KINDS, case_table, edge_plan, random_table
from tail_oracle_backend import tail_scores_table

# (R, K, S): the smallest shapes on both sides of every boundary of the follow-up paths.  K is 16 or at least 40 wherever
# the ordering plants of ``attribution_extras`` apply: at K = 16 a rank lists EVERY eligible kernel at top_n = 16 (the NaN
# and the zeros at the end of the order are visible), from K = 40 on the tie run is longer than any top_n.
FOLLOWUP_SHAPES = (
    (2, 2, 3),        # two ranks: the smallest table with a relative reference; k_colmin walks two rows
    (63, 16, 3),      # one row short of ...
    (64, 16, 3),      # ... the last R whose column minima k_colmin takes with one lane per column
    (65, 16, 3),      # the first R of k_colmin_part / k_colmin_finish: two chunks of 33 rows, the second one row short
    (100, 40, 5),     # two chunks of 50 rows: the eight-deep unrolled row loop runs twice, the second time with a remainder
    (129, 9, 4),      # three chunks (of 43 rows)
    (2049, 3, 3),     # 33 chunks of 64 rows capped to 32 chunks of 65; the last one holds 34
    (5, 1024, 3),     # the last K of k_attribute<256>: four ids per thread; the partial minima sit K floats into the scratch
    (5, 1025, 3),     # the first K of k_attribute<1024>: id 1024 is thread 0's second stride
    (4, 255, 255),    # one id short of a full stride of the 256-thread score kernels, in K and in S
    (4, 256, 256),    # exactly one stride
    (4, 257, 257),    # one id into the second stride
    (3, 0, 5),        # no kernel id: every GPU slot NaN, no column minimum over kernels is launched
    (3, 5, 0),        # no section
    (3, 1, 1),        # one column each
)
# tests/test_gpu_robust.py adds these to its own list
ROBUST_SHAPES = (
    (64, 3, 2),       # the last R of k_robust_cols<0> (64 columns x R rows staged in LDS) ...
    (65, 3, 2),       # ... and the first of k_robust_cols<256> (one workgroup per column)
    (1024, 2, 2),     # the last R of k_robust_cols<256> ...
    (1025, 2, 2),     # ... and the first of k_robust_cols<1024>
    (5, 32, 32),      # K + S = 64: one full tile of 64 columns
    (5, 32, 33),      # K + S = 65: one column into the second tile
)
TABLE_KINDS = ("live", "edge", "edge_common")
PLANE_KINDS = ("live", "edge")
# what edge_planes plants: COLUMN_KINDS with "plain" (a complete column of ordinary values) in the place of "zero_pos".  A
# family score is ref / v with ref the column's minimum, so ref <= v wherever both exist: a 0 in a column IS its minimum,
# x / 0 with x > 0 cannot be built and no family score is +inf (the +inf of these tests is an attribution ``score``, hmin / 0)
PLANE_COLUMN_KINDS = tuple("plain" if k == "zero_pos" else k for k in COLUMN_KINDS)

P_MISSING, P_HOLES = 0.15, 0.3


def _rng(tag, kind, R, K, S):
    return np.random.default_rng([R, K, S, tag, PLANE_KINDS.index(kind)])


def column_holes(rng, R, K, S, p_missing=P_MISSING, p_holes=P_HOLES):
    """[R, K+S] bool: absences drawn per column -- ``p_holes`` of the kernel columns and of the section columns (rounded
    down, picked at random) have holes, ``p_missing`` of their entries; the others are complete.  So at least half of a
    family's columns keep a reference whatever the seed.  ``p_holes = 1`` is the per-entry draw of ``random_table``."""
    holes = np.zeros(K + S, dtype=bool)
    for base, C in ((0, K), (K, S)):
        holes[base + rng.permutation(C)[: int(p_holes * C)]] = True
    return (rng.random((R, K + S)) < p_missing) & holes[None, :]


def live_table(rng, R, K, S, p_missing=P_MISSING, p_holes=P_HOLES):
    """``score_cases.random_table`` with the absences of ``column_holes``: most columns keep a relative reference."""
    T = random_table(rng, R, K, S, p_missing=0.0)
    KS = K + S
    missing = column_holes(rng, R, K, S, p_missing, p_holes)
    T[:, :KS][missing] = -1.0
    T[:, KS : 2 * KS][missing] = np.nan
    T[:, 2 * KS : 2 * KS + K][missing[:, :K]] = 0.0
    return T


# ---- the ordering plants of k_attribute ------------------------------------------------------------------------------------
EXTRA_FIRST_ID = 8  # ids 0-7 are edge_table's planted columns


def tie_ids(K):
    """The kernel ids of the tie run, a function of K alone (all at or above 14; empty below K = 16):

    * 14-19: neighbours, lanes 14-19 of wave 0;
    * 78, 79, 142, 206: lanes 14 / 15 of waves 1, 2 and 3;
    * 270, 271, 526, 527, 782: the same lanes one, two and three strides of k_attribute<256> on (one THREAD holds 14, 270,
      526 and 782; beyond K = 1024 thread 270 of k_attribute<1024> is lane 14 of wave 4);
    * K - 2, K - 1: the last ids, in the last stride (at K = 257 and K = 1025 id K - 1 is thread 0's second stride, the
      only one that stride has);
    * 1038, 1039, 1102 where K is large enough: thread 14's, 15's and 78's second stride of k_attribute<1024>;
    * then 20, 21, ... until the run holds 20 ids, which it does from K = 34 on (below that: every id from 14 up)."""
    if K < 16:
        return ()
    ids = {14, 15, 16, 17, 18, 19, 78, 79, 142, 206, 270, 271, 526, 527, 782, 1038, 1039, 1102, K - 2, K - 1}
    ids = {i for i in ids if 14 <= i < K}
    nxt = 20
    while len(ids) < 20 and nxt < K:
        ids.add(nxt)
        nxt += 1
    return tuple(sorted(ids))


def extras_plan(R, K):
    """Where ``attribution_extras`` plants what, a function of the shape alone; ``None`` where it plants nothing (K < 16 or
    R < 3).  ``rank`` holds the NaN and signed-zero kernels, ``tie_rank`` the tie run (another rank where the table has one
    to spare: a run that fills all 16 entries leaves room for nothing else); neither is ``edge_plan``'s ``lack`` or
    ``zero_w`` rank."""
    if K < 16 or R < 3:
        return None
    ep = edge_plan(R, K, 0, lacking_rank=True)
    pool = [r for r in range(R) if r not in (ep["lack"], ep["zero_w"])]
    rank, tie_rank = pool[0], pool[-1]
    anchor = next(r for r in range(R) if r not in (tie_rank, ep["lack"]))
    f = EXTRA_FIRST_ID
    return {"rank": rank, "tie_rank": tie_rank, "anchor": anchor, "lack": ep["lack"], "zero_w": ep["zero_w"],
            "zero_times_minus_inf": f, "zero_w_zero_zero": f + 1, "pos_w_zero_zero": f + 2, "minus_zero": f + 3,
            "plus_zero": f + 4, "minus_inf": f + 5, "tie": tie_ids(K)}


TIE_MED, TIE_MIN, TIE_W = 8.0, 2.0, 4096.0  # n_k = 4096 * (1 - 2 / 8) = 3072 in both families; no other n_k exceeds 1000


def attribution_extras(T, R, K, S):
    """Plant into ``T`` (in place; K >= 16 and R >= 3, else nothing) what the ordering of ``k_attribute`` has not seen.  On
    ``extras_plan``'s ``rank``, as (median, history minimum, weight):

    * id 8   (0, 1, 0)   individual score +inf, n_k = 0 * (1 - inf) = 0 * -inf: NaN;
    * id 9   (0, 0, 0)   0/0 with weight 0: NaN;
    * id 10  (0, 0, 7)   0/0 with a positive weight: NaN;
    * id 11  (4, 8, 0)   individual score 2, n_k = 0 * -1 = -0.0 ...
    * id 12  (4, 2, 0)   ... next to n_k = 0 * 0.5 = +0.0 at the HIGHER id: by value they tie and id 11 is listed first, by
      bit pattern +0.0 orders above -0.0 (in the relative family both are +0.0: a reference never exceeds a median);
    * id 13  (0, 1, 7)   individual score +inf, n_k = 7 * -inf = -inf: the last of the numbers, before every NaN;

    the weights of ``edge_plan``'s ``zero_w`` rank (the last one) are zeroed whatever the table's kind, so that a "live" table
    has a header with W = 0 too;

    and on ``tie_rank`` the tie run: ``tie_ids(K)`` all (8, 2, 4096), while every other rank that has kernels holds 2 to
    3.5 in these columns and ``anchor`` exactly 2 -- the run's n_k is 3072 in both families, above every other n_k of the
    rank (those are at most a weight, below 1000)."""
    plan = extras_plan(R, K)
    if plan is None:
        return T
    KS = K + S
    med, hmin, w = T[:, :K], T[:, KS : KS + K], T[:, 2 * KS : 2 * KS + K]
    r = plan["rank"]
    has_kernels = ~(med < 0).all(axis=1)  # (the kernel-less rank of an "edge" table stays so)
    for k in range(EXTRA_FIRST_ID, EXTRA_FIRST_ID + 6):  # these six columns are complete: whoever lacks one gets (3, 2, 5)
        gone = has_kernels & (med[:, k] < 0)
        med[gone, k], hmin[gone, k], w[gone, k] = 3.0, 2.0, 5.0
    for key, (m, h, wt) in (("zero_times_minus_inf", (0.0, 1.0, 0.0)), ("zero_w_zero_zero", (0.0, 0.0, 0.0)),
                            ("pos_w_zero_zero", (0.0, 0.0, 7.0)), ("minus_zero", (4.0, 8.0, 0.0)),
                            ("plus_zero", (4.0, 2.0, 0.0)), ("minus_inf", (0.0, 1.0, 7.0))):
        k = plan[key]
        med[r, k], hmin[r, k], w[r, k] = m, h, wt
    w[plan["zero_w"], :] = 0.0
    tie = np.array(plan["tie"], dtype=np.int64)
    for q in range(R):
        if not has_kernels[q]:
            continue
        m = 2.0 * (1.0 + (q % 7) / 8.0)
        med[q, tie], hmin[q, tie] = m, 0.75 * m
        if q != plan["zero_w"]:
            w[q, tie] = 1.0 + (q % 5)
    a = plan["anchor"]
    med[a, tie], hmin[a, tie] = TIE_MIN, 0.75 * TIE_MIN
    t = plan["tie_rank"]
    med[t, tie], hmin[t, tie], w[t, tie] = TIE_MED, TIE_MIN, TIE_W
    return T


def followup_table(kind, R, K, S):
    """The table of a follow-up parity case: ``live_table`` or ``score_cases.case_table("edge" | "edge_common")`` (unchanged,
    its own seeds), then ``attribution_extras``."""
    if kind == "live":
        T = live_table(_rng(0, kind, R, K, S), R, K, S)
    else:
        T = case_table(kind, R, K, S)
    return attribution_extras(T, R, K, S)


# ---- planes of the row families --------------------------------------------------------------------------------------------
def _plane0(rng, fam, R, KS):
    if fam.name == "tail":  # tails in microseconds
        return rng.lognormal(1.0, 0.5, (R, KS)).astype(np.float32)
    # shifts / excesses: 1.0 ("did not shift") on about half the rows, up to 3 on the others
    return np.where(rng.random((R, KS)) < 0.5, 1.0, rng.uniform(1.0, 3.0, (R, KS))).astype(np.float32)


def _other_planes(rng, planes, have):
    """Planes 1..P-1: 100-200 where plane 0 has a value (never a value plane 0 holds: a wrong pitch shows), -1 elsewhere."""
    R, P, KS = planes.shape
    for p in range(1, P):
        planes[:, p, :] = np.where(have, rng.uniform(100.0, 200.0, (R, KS)), -1.0)


def live_planes(rng, fam, R, K, S):
    """``[R][P][K+S]`` f32 planes of row family ``fam`` with the absences of ``column_holes``."""
    KS = K + S
    planes = np.full((R, fam.planes, KS), -1.0, dtype=np.float32)
    have = ~column_holes(rng, R, K, S)
    planes[:, 0, :] = np.where(have, _plane0(rng, fam, R, KS), -1.0)
    _other_planes(rng, planes, have)
    return planes


def plane_plan(R, K, S):
    """``edge_plan`` for planes: no rank lacks every kernel, and the kinds are those of ``PLANE_COLUMN_KINDS``."""
    plan = edge_plan(R, K, S, lacking_rank=False)
    for family in ("kernel", "section"):
        plan[family] = {("plain" if kind == "zero_pos" else kind): cr for kind, cr in plan[family].items()}
    return plan


def edge_planes(rng, fam, R, K, S):
    """``live_planes`` with the edge columns of ``plane_plan`` in plane 0 (a planted column is complete but for what the
    plant itself takes away):

    * ``zero_zero``  0.0 on one rank: the column's minimum, 0/0 = NaN there and a score of 0 everywhere else;
    * ``inf``        +inf on one rank: score 0; ``nan``: a NaN there, absent by ``v >= 0`` and ignored by the minimum;
    * ``nobody`` / ``one_rank``: no reference; ``equal``: 2 everywhere but 4 on one rank (scores exactly 1 and 0.5);
    * ``wide``       1e-15 against 1e15 on all others: scores of 1e-30."""
    KS = K + S
    planes = live_planes(rng, fam, R, K, S)
    v = planes[:, 0, :]
    fresh = _plane0(rng, fam, R, KS)
    plan = plane_plan(R, K, S)
    for family, base in (("kernel", 0), ("section", K)):
        for kind, (c, r) in plan[family].items():
            j = base + c
            gone = v[:, j] < 0
            v[gone, j] = fresh[gone, j]
            if kind == "zero_zero":
                v[r, j] = 0.0
            elif kind == "inf":
                v[r, j] = np.inf
            elif kind == "nan":
                v[r, j] = np.nan
            elif kind == "nobody":
                v[:, j] = -1.0
            elif kind == "one_rank":
                v[np.arange(R) != r, j] = -1.0
            elif kind == "equal":
                v[:, j] = 2.0
                if R >= 2:
                    v[r, j] = 4.0
            elif kind == "wide":
                v[:, j] = np.float32(1e15)
                v[r, j] = np.float32(1e-15)
    with np.errstate(invalid="ignore"):
        have = ~(v < 0)  # (a NaN is a value the rank reported)
    _other_planes(rng, planes, have)
    return planes


def followup_planes(kind, fam, R, K, S):
    """``(planes [R][P][K+S], exchange table [R][L])`` of a family-score case.  The weights of an "edge" case are those of
    ``case_table("edge")``: one rank's kernels all weigh zero (W = 0: a NaN GPU slot although it has kernels) and another
    rank's table row has no kernel at all -- its planes still have theirs, the score reads eligibility from the planes."""
    rng = _rng(10 + ("tail", "onset", "period", "episode").index(fam.name), kind, R, K, S)
    if kind == "live":
        return live_planes(rng, fam, R, K, S), live_table(rng, R, K, S)
    return edge_planes(rng, fam, R, K, S), case_table("edge", R, K, S)


def family_scores_table(fam, planes, T, K, S, first_rank=0, n_ranks=None):
    """The NumPy restatement of ``nvrx_<family>_score`` on planes ``[R][P][K+S]``."""
    if fam.name == "tail":
        return tail_scores_table(np.ascontiguousarray(planes[:, 0, :]), T, K, S, first_rank, n_ranks)
    table = {"onset": onset_scores_table, "period": period_scores_table, "episode": episode_scores_table}[fam.name]
    return table(planes, T, K, S, first_rank, n_ranks)


# ---- what keeps a parity test from passing vacuously (asserted on the CPU, counted on the GPU) ---------------------------
def live_columns(v, counted_out=()):
    """``(alive, counted)`` over the columns of ``v`` [R, C]: how many have a reference by the rule of ``k_colmin`` (no
    rank holds a negative value) among those not in ``counted_out``."""
    with np.errstate(invalid="ignore"):
        alive = ~(v < 0).any(axis=0)
    keep = np.ones(v.shape[1], dtype=bool)
    keep[list(counted_out)] = False
    return int((alive & keep).sum()), int(keep.sum())


def dead_by_plan(plan, family):
    """The columns (within the family) whose plants leave no reference on purpose."""
    return [plan[family][kind][0] for kind in ("nobody", "one_rank") if kind in plan[family]]

