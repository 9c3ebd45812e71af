"""Shared inputs of the score-route tests (tests/test_score_routes_host.py on the CPU, tests/test_gpu_score_routes.py on the
GPU): the shapes that pin every route of the score dispatch (``nvrx_score_route``), the table builders, and the one
comparison against the C oracle both files use."""
import numpy as np

from oracle import oracle

SINGLE, ROWS, ROWS_PRE, TILE16, TILE8 = 1, 2, 3, 4, 5  # NVRX_SCORE_ROUTE_* (include/nvrx_straggler.h)
ROUTE_NAMES = {SINGLE: "SINGLE", ROWS: "ROWS", ROWS_PRE: "ROWS_PRE", TILE16: "TILE16", TILE8: "TILE8"}

# (R, K, S) -> route, with 16-byte aligned result arrays: the smallest shapes of every route, both sides of each boundary
ROUTE_SHAPES = {
    (16, 13000, 40): SINGLE,   # 58 720 B of the 61 440 B a single workgroup may stage
    (64, 0, 94): SINGLE,       # the last section count of the single workgroup at 64 ranks
    (64, 0, 95): ROWS,         # ... and the first one past it
    (61, 5, 100): ROWS,        # R no multiple of the groups of eight score_colmin loads
    (64, 12248, 40): ROWS,     # 48 kernel ids per thread; the LDS minima take 49 152 B exactly
    (1, 0, 12288): ROWS,       # the publication of a lone workgroup, at the 48 KB boundary
    (8, 0, 767): ROWS,
    (1, 0, 12289): ROWS_PRE,   # one float past 48 KB of LDS minima
    (2, 15400, 0): ROWS_PRE,   # one chunk of two rows in k_colmin_part
    (65, 3, 614): ROWS_PRE,    # the first S no tile takes
    (65, 3, 306): TILE16,      # the last S of the 16-rank tile; the last tile holds one rank
    (100, 7, 9): TILE16,
    (65, 3, 307): TILE8,       # the first S of the 8-rank tile
    (70, 0, 613): TILE8,       # the last one: 49 120 B of 49 152; the last tile holds six ranks
}

# scratch regrowth (tests/test_gpu_score_routes.py): a ROWS_PRE launch, then a TILE16 one that needs a larger buffer
REGROW_SHAPES = ((65, 3, 614), (1024, 100, 64))

# nvrx_score's thresholds {gpu_rel, section_rel, gpu_indiv, section_indiv} in the GPU tests.  The two section thresholds
# are exact in f32, and edge_table plants section scores that EQUAL them: the compare is strict, those are not flagged
THRESHOLDS = (0.8, 0.5, 0.9, 0.75)
COMBOS = ((True, True), (True, False), (False, True))  # (do_indiv, do_rel)
GPU_SCORE_RTOL = 2e-6   # GPU-score columns: f64 sums in another order than the oracle's serial loop
FLAG_MARGIN = 4e-6      # no oracle GPU score may sit this close (relative) to its threshold: then every flag is decided


def threshold_columns(S, thr=THRESHOLDS):
    """The threshold of every column of a score row {gpu_indiv, gpu_rel, indiv[S], rel[S]}."""
    return np.concatenate([[thr[2], thr[0]], np.full(S, thr[3]), np.full(S, thr[1])])


def random_table(rng, R, K, S, p_missing=0.15):
    """An exchanged table [R][NVRX_TABLE_LEN(K, S)]: lognormal medians, history minima at 50-100 % of them, ``p_missing`` of
    the entries absent (median -1, minimum NaN, weight 0), every rank with all its names."""
    L = oracle.table_len(K, S)
    KS = K + S
    T = np.zeros((R, L), dtype=np.float32)
    med = rng.lognormal(1.0, 0.5, (R, KS)).astype(np.float32)
    hmin = (med * rng.uniform(0.5, 1.0, (R, KS))).astype(np.float32)
    missing = rng.random((R, KS)) < p_missing
    med[missing] = -1.0
    hmin[missing] = np.nan
    T[:, :KS] = med
    T[:, KS : 2 * KS] = hmin
    w = rng.uniform(1, 1000, (R, K)).astype(np.float32)
    w[missing[:, :K]] = 0.0
    T[:, 2 * KS : 2 * KS + K] = w
    T[:, L - 1] = 1.0
    return T


# what edge_table plants into single columns, in the order the section columns take them (the kernel columns take them
# in reverse, so a table with K + S >= 8 holds every kind even when neither family has eight columns)
COLUMN_KINDS = ("zero_zero", "zero_pos", "inf", "nan", "nobody", "one_rank", "equal", "wide")


def edge_plan(R, K, S, lacking_rank=True):
    """Where ``edge_table`` plants what -- a function of the shape alone, so a test can say where NaN, inf and 0 must appear:
    ``{"kernel": {kind: (column within the family, rank)}, "section": {...}, "lack": rank or None, "zero_w": rank or None}``."""
    lack = R // 2 if (lacking_rank and R >= 2 and K > 0) else None
    zero_w = (R - 1 if R >= 3 else 0) if (R >= 2 and K > 0) else None  # (beyond 64 ranks: in the last tile)
    plan = {"lack": lack, "zero_w": zero_w, "kernel": {}, "section": {}}
    # a column's special rank: never the rank that lacks every kernel, and for sections counted from the last rank down
    # (beyond 64 ranks those sit in the last tiles)
    pool = [r for r in range(R) if r != lack]
    for c, kind in enumerate(COLUMN_KINDS):
        if c < S:
            plan["section"][kind] = (c, pool[-1 - (c * 3) % len(pool)])
    for c, kind in enumerate(reversed(COLUMN_KINDS)):
        if c < K:
            plan["kernel"][kind] = (c, pool[(c * 7 + 1) % len(pool)])
    return plan


def edge_table(rng, R, K, S, lacking_rank=True):
    """``random_table``'s layout with the values planted at which scoring goes wrong, in the kernel columns and in the section
    columns (``edge_plan`` says where; a family with fewer than eight columns takes the first kinds that fit):

    * ``zero_zero``  a median of 0.0 whose history minimum is 0.0 too: 0/0, NaN;
    * ``zero_pos``   a median of 0.0 with a positive minimum: an infinite individual score, never flagged;
    * ``inf``        a median of +inf: score 0, flagged;
    * ``nan``        a NaN median: absent by the ``med >= 0`` rule and ignored by the column minimum;
    * ``nobody``     a column every rank lacks: relative NaN for all;
    * ``one_rank``   a column exactly one rank has: its individual score stands (exactly 0.75, the section threshold of
      ``THRESHOLDS``: not flagged), the relative one is NaN for it too (the -1 of the others wins the minimum,
      reporting.py:289-295);
    * ``equal``      the same median on every rank (ties in the minimum: relative score exactly 1) but one, at exactly twice
      that (relative score exactly 0.5, the section threshold: not flagged);
    * ``wide``       1e-15 on one rank against 1e15 on all others: a relative score of 1e-30;
    * a rank whose kernels all weigh zero (0/0: NaN GPU scores although it has kernels), a rank that lacks every kernel
      (relative GPU score NaN for everybody; ``lacking_rank=False`` leaves it out, so the relative GPU scores of the other
      plants stay comparable), and the names word 0 on the last rank only -- beyond 64 ranks that is a rank ``score_meta``
      reaches on its second stride, in the last tile.

    Every column has its own scale and the medians lie between 1e-15 and 1e15, so every quotient stays a normal f32.

    Deliberately left out: ``-0.0`` medians (the minimum of -0.0 and 0.0 depends on the order of comparison, so oracle and
    kernel may legitimately differ in the sign of an infinity), and quotients in the f32 subnormal range (the f32 division
    of the single-workgroup kernel and the f64 quotient elsewhere need not agree there, and no timing in microseconds lives
    there)."""
    L = oracle.table_len(K, S)
    KS = K + S
    # a column's medians lie within [scale / 25, scale]
    scale = 10.0 ** rng.uniform(np.log10(25e-15), 15.0, KS)
    if KS >= 2:  # both ends of the range are reached
        lo = int(rng.integers(0, KS))
        scale[lo] = 25e-15
        scale[(lo + 1 + int(rng.integers(0, KS - 1))) % KS] = 1e15
    med = (rng.lognormal(0.0, 0.5, (R, KS)).clip(0.2, 5.0) * scale[None, :] / 5.0).astype(np.float32)
    hmin = (med.astype(np.float64) * rng.uniform(0.5, 1.0, (R, KS))).astype(np.float32)
    # An absent entry makes its whole column's relative scores NaN (the -1 wins the minimum), so only three columns in
    # ten have any: the others keep relative scores to compare
    missing = (rng.random((R, KS)) < 0.15) & (rng.random(KS) < 0.3)[None, :]
    w = rng.uniform(1, 1000, (R, K)).astype(np.float32)
    med[missing] = -1.0
    hmin[missing] = np.nan
    w[missing[:, :K]] = 0.0

    plan = edge_plan(R, K, S, lacking_rank)
    for family, base in (("kernel", 0), ("section", K)):
        for kind, (c, r) in plan[family].items():
            j = base + c
            others = np.arange(R) != r
            pow2 = np.float32(2.0 ** np.floor(np.log2(scale[j])))  # (exact halves and quarters)
            gone = med[:, j] < 0  # a planted column is complete but for what the plant itself takes away
            med[gone, j] = np.float32(scale[j] / 5.0)
            hmin[gone, j] = np.float32(scale[j] / 10.0)
            if kind in ("zero_zero", "zero_pos", "inf", "nan"):
                med[r, j] = {"zero_zero": 0.0, "zero_pos": 0.0, "inf": np.inf, "nan": np.nan}[kind]
                hmin[r, j] = 0.0 if kind == "zero_zero" else np.float32(0.75 * scale[j] / 5.0)
                if kind == "inf" and R >= 2:  # somebody else has the column: its minimum is finite
                    med[(r + 1) % R, j], hmin[(r + 1) % R, j] = np.float32(scale[j] / 2.0), np.float32(scale[j] / 4.0)
            elif kind == "nobody":
                med[:, j], hmin[:, j] = -1.0, np.nan
            elif kind == "one_rank":
                med[others, j], hmin[others, j] = -1.0, np.nan
                med[r, j] = pow2
                hmin[r, j] = pow2 * np.float32(0.75)
            elif kind == "equal":
                med[:, j] = pow2
                if R >= 2:
                    med[r, j] = pow2 * np.float32(2.0)
                hmin[:, j] = (med[:, j] * rng.uniform(0.5, 1.0, R)).astype(np.float32)
            elif kind == "wide":
                med[:, j], hmin[:, j] = np.float32(1e15), np.float32(0.9e15)
                med[r, j], hmin[r, j] = np.float32(1e-15), np.float32(0.9e-15)
            if family == "kernel":
                present = med[:, j] >= 0  # (False for NaN and -1)
                w[:, c] = np.where(present, np.maximum(w[:, c], 1.0), 0.0)
    if plan["zero_w"] is not None:
        w[plan["zero_w"], :] = 0.0
    if plan["lack"] is not None:
        med[plan["lack"], :K], hmin[plan["lack"], :K], w[plan["lack"], :] = -1.0, np.nan, 0.0

    T = np.zeros((R, L), dtype=np.float32)
    T[:, :KS] = med
    T[:, KS : 2 * KS] = hmin
    T[:, 2 * KS : 2 * KS + K] = w
    T[:, L - 1] = 1.0
    T[R - 1, L - 1] = 0.0
    return T


TABLE_KINDS = ("random", "edge", "edge_common")


def case_table(kind, R, K, S):
    """The table of a parity case.  The seeds are chosen so that no oracle GPU score sits within ``FLAG_MARGIN`` of its
    threshold (tests/test_score_routes_host.py checks that), which is what lets the GPU test demand every flag."""
    rng = np.random.default_rng([R, K, S, TABLE_KINDS.index(kind)])
    if kind == "random":
        return random_table(rng, R, K, S)
    return edge_table(rng, R, K, S, lacking_rank=(kind == "edge"))


def expected_flags(exp, S, thr=THRESHOLDS):
    """Flags of the ORACLE's scores: strict ``<``, NaN and +inf never flagged (reporting.py:84-151)."""
    with np.errstate(invalid="ignore"):
        return (exp.astype(np.float64) < threshold_columns(S, thr)[None, :]).astype(np.uint8)


def gpu_scores_near_threshold(exp, S, thr=THRESHOLDS):
    """How many oracle GPU scores (columns 0-1) lie within ``FLAG_MARGIN * threshold`` of their threshold."""
    t = threshold_columns(S, thr)[None, :2]
    with np.errstate(invalid="ignore"):
        return int((np.abs(exp[:, :2].astype(np.float64) - t) <= FLAG_MARGIN * t).sum())


def compare_scores(got, exp):
    """A kernel's score rows against the oracle's.  Section columns (one f64 division rounded to f32): bit-identical, NaN
    compared by NaN-ness.  GPU-score columns: the same NaN-ness, the same infinities, finite values within
    ``GPU_SCORE_RTOL``.  Returns the largest relative GPU-score difference seen."""
    assert got.shape == exp.shape and got.dtype == exp.dtype == np.float32
    nan = np.isnan(exp)
    assert np.array_equal(np.isnan(got), nan), np.argwhere(np.isnan(got) != nan)[:8]
    sec_ok = ~nan[:, 2:]
    gs, es = got[:, 2:][sec_ok].view(np.uint32), exp[:, 2:][sec_ok].view(np.uint32)
    assert np.array_equal(gs, es), (int((gs != es).sum()), np.argwhere(got[:, 2:].view(np.uint32) != exp[:, 2:].view(np.uint32))[:8])
    g, e = got[:, :2].astype(np.float64), exp[:, :2].astype(np.float64)
    inf = np.isinf(e)
    assert np.array_equal(np.isinf(g), inf) and np.array_equal(g[inf], e[inf])
    fin = np.isfinite(e)
    if not fin.any():
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(e[fin] != 0.0, np.abs(g[fin] - e[fin]) / np.abs(e[fin]), np.where(g[fin] == 0.0, 0.0, np.inf))
    worst = float(rel.max())
    assert worst <= GPU_SCORE_RTOL, worst
    return worst
