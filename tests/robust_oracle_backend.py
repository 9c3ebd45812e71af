"""Robust scores for the CPU checker backend, and the NumPy restatement the robust tests compare against -- TEST
INFRASTRUCTURE, lives outside the product.

``robust_columns`` / ``robust_scores_table`` restate the definitions of include/nvrx_straggler.h (``nvrx_robust_score``) in
NumPy; ``RobustOracleBackend`` / its rings are the checker with tails (``TailOracleBackend``) plus kernel attribution plus
``robust_score`` / ``report_robust`` built on them, so that the host side of the feature (option plumbing, collectives,
names, lifetime, pickling, all three follow-ups together) runs on a box without a GPU.
"""
import numpy as np

from attribution_oracle_backend import AttributionOracleBackend
from oracle_backend import OracleBackend, OracleRings, OracleRingsFused
from tail_oracle_backend import TailOracleBackend, TailOracleRings, TailOracleRingsFused, f2key, key2f

NAN32 = np.float32(np.nan)
NAN_BITS = NAN32.view(np.uint32)


def lower_median_by_key(keys):
    """The element of rank (n-1) >> 1 of the uint32 keys, sorted ascending."""
    keys = np.sort(np.asarray(keys, dtype=np.uint32))
    return keys[(keys.size - 1) >> 1]


def robust_columns(T, K, S, min_ranks, floor_rel):
    """``[K+S, 4]`` uint32 column records {f32 ctr, f32 mad, f32 scale, u32 n} of the f32 table ``T`` [R, L]."""
    T = np.asarray(T, dtype=np.float32)
    KS = K + S
    out = np.zeros((KS, 4), dtype=np.uint32)
    f = out.view(np.float32)
    floor_rel = np.float32(floor_rel)
    for c in range(KS):
        v = T[:, c]
        with np.errstate(invalid="ignore"):
            v = v[v >= 0]  # the -1 sentinel and NaN are absent
        n = v.size
        out[c, 3] = n
        if n == 0 or n < min_ranks:
            out[c, :3] = NAN_BITS
            continue
        ctr = key2f(lower_median_by_key(f2key(v)))
        with np.errstate(invalid="ignore", over="ignore"):
            dev = (v - np.float32(ctr)).astype(np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)  # fabsf; NaN above +inf
            mad = np.uint32(lower_median_by_key(dev)).view(np.float32)
            scale = np.fmax(np.float32(1.4826) * mad, floor_rel * np.float32(ctr)).astype(np.float32)
        f[c, 0], f[c, 1], f[c, 2] = ctr, mad, scale
    return out


def robust_scores_table(T, K, S, first_rank=0, n_ranks=None, min_ranks=4, floor_rel=0.02):
    """``(cols [K+S, 4] uint32, scores [n_ranks, 2, 1 + S] f32)``: plane 0 the ratios ctr / v, plane 1 the z (v - ctr) /
    scale; slot 0 of each the weighted mean over the eligible kernels in f64."""
    T = np.asarray(T, dtype=np.float32)
    R, KS = T.shape[0], K + S
    n_ranks = R - first_rank if n_ranks is None else n_ranks
    cols = robust_columns(T, K, S, min_ranks, floor_rel)
    f = cols.view(np.float32)
    ctr, scale = f[:, 0].astype(np.float64), f[:, 2].astype(np.float64)
    has_ref = (cols[:, 3] >= min_ranks) & (cols[:, 3] > 0)
    out = np.full((n_ranks, 2, 1 + S), NAN32, dtype=np.float32)
    for i in range(n_ranks):
        row = T[first_rank + i]
        v = row[:KS].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            ok = (row[:KS] >= 0) & has_ref
            ratio = ctr / v
            z = (v - ctr) / scale
            out[i, 0, 1:] = np.where(ok[K:], ratio[K:], np.nan).astype(np.float32)
            out[i, 1, 1:] = np.where(ok[K:], z[K:], np.nan).astype(np.float32)
            elig = ok[:K]
            if elig.any():
                w = row[2 * KS : 2 * KS + K].astype(np.float64)[elig]
                out[i, 0, 0] = np.float32((w * ratio[:K][elig]).sum() / w.sum())
                out[i, 1, 0] = np.float32((w * z[:K][elig]).sum() / w.sum())
    return cols, out


class _OracleRobust:
    def __init__(self, rec, first_rank, n_ranks):
        self._rec = rec
        self.first_rank, self.n_ranks = first_rank, n_ranks
        self.reads = 0

    def records(self):
        self.reads += 1
        return self._rec


def _robust(backend, ws, table, first_rank, n_ranks, min_ranks, floor_rel):
    backend.robust_calls += 1
    n_ranks = ws.R - first_rank if n_ranks is None else n_ranks
    backend.robust_args.append((first_rank, n_ranks, min_ranks, floor_rel))
    h = _OracleRobust(robust_scores_table(table.numpy().copy(), ws.K, ws.S, first_rank, n_ranks, min_ranks, floor_rel),
                      first_rank, n_ranks)
    backend.robust_handles.append(h)
    return h


class _RobustRingsMixin:
    """What the product's rings add for a one-call report: the follow-ups on the table that report used."""

    def report_fused(self, ws, rows_active, stats_rows, do_indiv, do_rel, thresholds, direct=None, **kw):
        self._last = (ws.table if direct is not None else ws.send, do_indiv, do_rel)
        return super().report_fused(ws, rows_active, stats_rows, do_indiv, do_rel, thresholds, direct, **kw)

    def report_robust(self, ws, first_rank=0, n_ranks=None, min_ranks=4, floor_rel=0.02):
        return _robust(self.backend, ws, self._last[0], first_rank, n_ranks, min_ranks, floor_rel)

    def report_attribute(self, ws, top_n, first_rank=0, n_ranks=None):
        table, do_indiv, do_rel = self._last
        return self.backend.attribute(ws, table, top_n, do_indiv, do_rel, first_rank, n_ranks)


class RobustOracleRings(TailOracleRings):
    pass


class RobustOracleRingsFused(_RobustRingsMixin, TailOracleRingsFused):
    pass


class RobustOracleBackend(TailOracleBackend):
    """The CPU checker with all three follow-ups: tails, kernel attribution and robust scores (computed at enqueue time)."""

    name = "oracle-test+robust"

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.attribute_calls = 0
        self.robust_calls = 0
        self.robust_args = []
        self.robust_handles = []

    attribute = AttributionOracleBackend.attribute

    def make_rings(self, local_ranks, rows_per_rank, ring_cap):
        cls = RobustOracleRingsFused if self.emulate_fused else RobustOracleRings
        return cls(self, local_ranks, rows_per_rank, ring_cap)

    def robust_score(self, ws, table, first_rank=0, n_ranks=None, min_ranks=4, floor_rel=0.02):
        return _robust(self, ws, table, first_rank, n_ranks, min_ranks, floor_rel)


class _RaisingRings(OracleRings):
    def report_robust(self, *a, **kw):
        self.backend.robust_calls += 1
        raise AssertionError("report_robust() called although robust_scores is off")


class _RaisingRingsFused(OracleRingsFused):
    report_robust = _RaisingRings.report_robust


class CountingRobustBackend(OracleBackend):
    """The plain checker plus ``robust_score`` / ``report_robust`` that only count and raise: with the option off nobody may
    call them."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.robust_calls = 0

    def make_rings(self, local_ranks, rows_per_rank, ring_cap):
        cls = _RaisingRingsFused if self.emulate_fused else _RaisingRings
        return cls(self, local_ranks, rows_per_rank, ring_cap)

    def robust_score(self, *a, **kw):
        self.robust_calls += 1
        raise AssertionError("robust_score() called although robust_scores is off")
