"""Kernel attribution for the CPU checker backend, and the NumPy references the attribution tests compare against --
TEST INFRASTRUCTURE, lives outside the product.

``attribute_table`` is the formula of include/nvrx_straggler.h (``nvrx_attribute``) in NumPy f64 on an exchange table;
``AttributionOracleBackend`` is ``OracleBackend`` plus ``attribute`` built on it, so that the host side of the feature
(option plumbing, coverage, names, lifetime, pickling) runs on a box without a GPU.  ``expected_from_summaries`` derives the
same quantities from a golden scenario's own summaries, without any table.
"""
import numpy as np

from oracle_backend import OracleBackend

NAN32 = np.float32(np.nan)


def rank_by_loss(ids, lost):
    """Positions of ``ids`` ordered by descending ``lost`` BY VALUE, ties by the lower id: ``-0.0`` and ``+0.0`` tie, a NaN
    comes after -inf whatever its sign bit (the ordering rule of ``nvrx_attribute``, include/nvrx_straggler.h)."""
    ids = np.asarray(ids)
    lost = np.asarray(lost, dtype=np.float64)
    return np.lexsort((ids, -lost))


def column_minima(med):
    """``[K]`` f32 references of the relative family: the rule of ``k_colmin`` (``v < m``: a NaN median never wins, the -1 of
    an absent entry does), NaN where some rank lacks the kernel -- as ``nvrx_score`` takes them."""
    med = np.asarray(med, dtype=np.float32)
    m = np.full(med.shape[1], np.inf, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        for r in range(med.shape[0]):
            m = np.where(med[r] < m, med[r], m)
        return np.where(m >= 0, m, NAN32).astype(np.float32)


def loss_terms(T, K, S, r, fam, minmed=None):
    """``(ids, s, n, w)`` of rank ``r``'s eligible kernels in family ``fam`` (0 individual, 1 relative), f64, unordered: the
    scores s_k = ref_k / med_k and the lost microseconds n_k = w_k * (1 - s_k) exactly as the formula produces them (a zero
    n_k keeps its sign here; the records report it as +0.0)."""
    T = np.asarray(T, dtype=np.float32)
    KS = K + S
    med, hmin, w = T[:, :K], T[:, KS : KS + K], T[:, 2 * KS : 2 * KS + K]
    ref = (column_minima(med) if minmed is None else minmed) if fam else hmin[r]
    with np.errstate(invalid="ignore", divide="ignore"):
        elig = med[r] >= 0
        if fam:
            elig &= ~np.isnan(ref)
        ids = np.flatnonzero(elig)
        s = ref[ids].astype(np.float64) / med[r, ids].astype(np.float64)
        wk = w[r, ids].astype(np.float64)
        return ids, s, wk * (1.0 - s), wk


def attribute_table(T, K, S, top_n, do_indiv, do_rel, first_rank=0, n_ranks=None):
    """``[n_ranks, 2, 1 + top_n, 4]`` uint32 records (family 0 individual, 1 relative) of the f32 table ``T`` [R, L]."""
    T = np.asarray(T, dtype=np.float32)
    R = T.shape[0]
    n_ranks = R - first_rank if n_ranks is None else n_ranks
    KS = K + S
    minmed = column_minima(T[:, :K])
    out = np.zeros((n_ranks, 2, 1 + top_n, 4), dtype=np.uint32)
    f32 = out.view(np.float32)
    i32 = out.view(np.int32)
    f32[:, :, :, :] = NAN32
    i32[:, :, 1:, 0] = -1
    out[:, :, 0, 2] = 0
    f32[:, :, 0, 3] = 0.0
    for i in range(n_ranks):
        r = first_rank + i
        for fam, on in ((0, do_indiv), (1, do_rel)):
            if not on:
                continue
            ids, s, n, wk = loss_terms(T, K, S, r, fam, minmed)
            if ids.size == 0:
                continue
            W = wk.sum()
            order = rank_by_loss(ids, n)[:top_n]
            with np.errstate(invalid="ignore", divide="ignore"):
                n = n + 0.0  # (a zero n_k is reported as +0.0; NaN stays NaN)
                f32[i, fam, 0, 0] = n.sum() / W
                f32[i, fam, 0, 1] = n[order].sum() / W
                out[i, fam, 0, 2] = ids.size
                f32[i, fam, 0, 3] = W
                for j, p in enumerate(order):
                    i32[i, fam, 1 + j, 0] = ids[p]
                    f32[i, fam, 1 + j, 1] = n[p] / W
                    f32[i, fam, 1 + j, 2] = s[p]
                    f32[i, fam, 1 + j, 3] = n[p]
    return out


class _OracleAttribution:
    def __init__(self, records, first_rank, n_ranks, top_n):
        self._records = records
        self.first_rank, self.n_ranks, self.top_n = first_rank, n_ranks, top_n

    def records(self):
        return self._records


class AttributionOracleBackend(OracleBackend):
    """The CPU checker with kernel attribution (computed at enqueue time, like its scores)."""

    name = "oracle-test+attribution"

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.attribute_calls = 0

    def attribute(self, ws, table, top_n, do_indiv, do_rel, first_rank=0, n_ranks=None):
        self.attribute_calls += 1
        n_ranks = ws.R - first_rank if n_ranks is None else n_ranks
        rec = attribute_table(table.numpy().copy(), ws.K, ws.S, top_n, do_indiv, do_rel, first_rank, n_ranks)
        return _OracleAttribution(rec, first_rank, n_ranks, top_n)


class CountingOracleBackend(OracleBackend):
    """The plain checker plus an ``attribute`` that only counts: with the option off nobody may call it."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.attribute_calls = 0

    def attribute(self, *a, **kw):
        self.attribute_calls += 1
        raise AssertionError("attribute() called although kernel_attribution is off")


def expected_from_summaries(steps, t, rank, world, kernel_ids, family):
    """What ``explain_gpu_scores()[family][rank]`` must say at step ``t`` of a golden scenario (``steps[t][rank] = (section
    summaries, kernel summaries)``), from the summaries alone: ``None`` where the reference's score is NaN, else ``(deficit,
    [(name, share, score, lost_us), ...])`` over ALL eligible kernels, ranked.  Inputs pass through f32 as the exchange table's do."""
    def kernels(tt, r):
        return {k: v for k, v in steps[tt][r][1].items() if "ncclDev" not in k}

    mine = kernels(t, rank)
    f = np.float32
    if family == "relative":
        others = [kernels(t, r) for r in range(world)]
        if any(not o for o in others):
            return None  # a rank without kernels: NaN everywhere (reporting.py:289,295)
        common = [k for k in mine if all(k in o for o in others)]
        ref = {k: min(f(o[k]["MED"]) for o in others) for k in common}
    else:
        ref = {k: min(f(kernels(tt, rank)[k]["MED"]) for tt in range(t + 1) if k in kernels(tt, rank)) for k in mine}
    names = list(ref)
    if not names:
        return None
    ids = np.array([kernel_ids[k] for k in names])
    med = np.array([f(mine[k]["MED"]) for k in names], dtype=np.float64)
    w = np.array([f(mine[k]["NUM"] * mine[k]["AVG"]) for k in names], dtype=np.float64)
    s = np.array([ref[k] for k in names], dtype=np.float64) / med
    n = w * (1.0 - s)
    W = w.sum()
    order = rank_by_loss(ids, n)
    return float(n.sum() / W), [(names[p], float(n[p] / W), float(s[p]), float(n[p])) for p in order]
