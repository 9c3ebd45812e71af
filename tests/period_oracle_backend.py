"""Period scores for the CPU checker backend, and the NumPy restatement the period tests compare against -- TEST
INFRASTRUCTURE, lives outside the product.

``fold_curves`` / ``row_period`` / ``period_excess`` / ``period_scores_table`` restate the definitions of
include/nvrx_straggler.h (``nvrx_row_period``, ``nvrx_period_score``) in NumPy: one float64 ``bincount`` per candidate period
over the samples in time order, pivoted on the first one.  ``PeriodOracleBackend`` / ``PeriodOracleRings`` are
``OnsetOracleBackend`` / ``OnsetOracleRings`` plus ``period_local`` / ``period_score`` built on them, so that the host side of
the feature (option plumbing, collectives, names, lifetime, pickling) runs on a box without a GPU.
"""
import numpy as np
import torch

from onset_oracle_backend import OnsetOracleBackend, _OnsetRingsMixin, time_order
from oracle_backend import OracleBackend, OracleRings, OracleRingsFused
from tail_oracle_backend import _TailRingsMixin, tail_scores_table

NAN32 = np.float32(np.nan)
PLANES = 7  # {e, peak, rest, strength, period, ago, n}
MIN_CYCLES = 4
BAR = 0.95
REC = [("period", np.uint32), ("ago", np.uint32), ("peak", np.float32), ("rest", np.float32), ("strength", np.float32)]


def period_cap(n, max_period):
    """Pmax = min(max_period, n / 4), integer division."""
    return min(int(max_period), int(n) // MIN_CYCLES)


def fold_curves(X, max_period):
    """``(a [rows, Pmax - 1], T [rows], SST [rows])`` of rows of equal length given in time order, ``a[:, P - 2]`` the adjusted
    share of the row's variance that the fold at P explains, in float64 over values pivoted on each row's first sample."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float32))
    rows, n = X.shape
    d = X.astype(np.float64) - X[:, :1].astype(np.float64)
    pmax = period_cap(n, max_period)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        T = d.sum(axis=1)
        sst = ((d - (T / n)[:, None]) ** 2).sum(axis=1)
        a = np.zeros((rows, max(pmax - 1, 0)), dtype=np.float64)
        base = np.arange(rows)[:, None]
        i = np.arange(n)
        for P in range(2, pmax + 1):
            phase = i % P
            S = np.bincount((base * P + phase[None, :]).ravel(), weights=d.ravel(), minlength=rows * P).reshape(rows, P)
            cnt = np.bincount(phase, minlength=P).astype(np.float64)
            B = (S * S / cnt[None, :]).sum(axis=1) - T * T / n
            a[:, P - 2] = 1.0 - (1.0 - B / sst) * (n - 1.0) / (n - P)
    return a, T, sst


def choose(curve):
    """``(P*, a_max)`` of one row's curve (``curve[P - 2]``); P* is 0 when no period explains anything."""
    if curve.size == 0:
        return 0, 0.0
    a_max = float(curve.max())
    if not a_max > 0.0:
        return 0, a_max
    return 2 + int(np.argmax(curve >= BAR * a_max)), a_max  # (the first at or above the bar)


def phase_means(x, P):
    """``(S_f, n_f)`` of one row in time order at period P."""
    d = x.astype(np.float64) - np.float64(x[0])
    phase = np.arange(x.size) % P
    return np.bincount(phase, weights=d, minlength=P), np.bincount(phase, minlength=P).astype(np.float64)


def record_at(x, P, T, strength):
    """The record of a row in time order whose period is P > 0, and its slow phase."""
    n = x.size
    S, cnt = phase_means(x, P)
    f = int(np.argmax(S / cnt))  # (the first of equals)
    x0 = np.float64(x[0])
    rec = (P, (n - 1 - f) % P, np.float32(x0 + S[f] / cnt[f]), np.float32(x0 + (T - S[f]) / (n - cnt[f])), np.float32(strength))
    return rec, f


def row_period_one(x, max_period, curve=None, T=None, sst=None):
    """``(period, ago, peak, rest, strength)`` of one row given in time order (n >= 1), the curve ``a[P - 2]`` over the
    candidate periods (None where the row has none or is constant or not finite) and the slow phase (None without a period)."""
    n = x.size
    if curve is None:
        a, T, sst = fold_curves(x[None, :], max_period)
        curve, T, sst = a[0], T[0], sst[0]
    if not (np.isfinite(T) and np.isfinite(sst)):
        return (0, 0, NAN32, NAN32, NAN32), None, None
    mean = np.float32(np.float64(x[0]) + T / n)
    if period_cap(n, max_period) < 2:
        return (0, 0, mean, mean, np.float32(0.0)), None, None
    if sst == 0.0:
        return (0, 0, np.float32(x[0]), np.float32(x[0]), np.float32(0.0)), None, None
    P, _ = choose(curve)
    if P == 0:
        return (0, 0, mean, mean, np.float32(0.0)), curve, None
    rec, f = record_at(x, P, T, curve[P - 2])
    return rec, curve, f


def row_period(samples, counts, max_period, starts=None):
    """``[rows]`` structured records ``{period, ago u32, peak, rest, strength f32}`` of every row (absent: {0, 0, -1, -1, -1}),
    per row the curve over its candidate periods (or None), the slow phase (or None) and the row in time order (or None).
    Rows of equal count are folded together."""
    samples = np.asarray(samples, dtype=np.float32)
    rows, stride = samples.shape
    out = np.zeros(rows, dtype=REC)
    curves, phases, ordered = [None] * rows, [None] * rows, [None] * rows
    ns = [min(int(c), stride) for c in np.asarray(counts).tolist()]
    for n in sorted(set(ns)):
        idx = [r for r in range(rows) if ns[r] == n]
        if n == 0:
            for r in idx:
                out[r] = (0, 0, -1.0, -1.0, -1.0)
            continue
        X = np.stack([time_order(samples[r], n, 0 if starts is None else starts[r]) for r in idx])
        a, T, sst = fold_curves(X, max_period)
        for j, r in enumerate(idx):
            out[r], curves[r], phases[r] = row_period_one(X[j], max_period, a[j], T[j], sst[j])
            ordered[r] = X[j]
    return out, curves, phases, ordered


def period_excess(period, peak, rest, strength, min_strength):
    """The effective excess of a record: f32 of the f64 quotient peak / rest where the beat is a convincing slow-down."""
    peak, rest, strength = np.float32(peak), np.float32(rest), np.float32(strength)
    with np.errstate(invalid="ignore"):
        if period > 0 and strength >= np.float32(min_strength) and peak > rest and rest > 0:
            return np.float32(np.float64(peak) / np.float64(rest))
    return np.float32(1.0)


def period_scores_table(periods, table, K, S, first_rank=0, n_ranks=None):
    """``[n_ranks, 1 + S]`` f32 {GPU period score, section period scores} from the period table ``periods`` [R, 7, K+S] (plane
    0: the effective excesses) and the weights in the exchange table ``table`` [R, L]: the tail scores' arithmetic on plane 0."""
    periods = np.asarray(periods, dtype=np.float32)
    return tail_scores_table(np.ascontiguousarray(periods[:, 0, :]), table, K, S, first_rank, n_ranks)


def ring_periods(rings, ws_K, ws_S, max_period, min_strength, rows_active=0):
    """[local_ranks, 7, K+S] period planes of NumPy rings (``OracleRings``), packed by gid."""
    KS = ws_K + ws_S
    out = np.full((rings.local_ranks, PLANES, KS), -1.0, dtype=np.float32)
    cap = rings.ring_cap
    active = rows_active or rings.rows_per_rank
    for lr in range(rings.local_ranks):
        for row in range(active):
            r = lr * rings.rows_per_rank + row
            g = int(rings.gid[r])
            total = int(rings.total[r])
            n = min(total, cap)
            if 0 <= g < KS and n > 0:
                start = total % cap if total > cap else 0
                (period, ago, peak, rest, strength), _, _ = row_period_one(time_order(rings.samples[r], n, start), max_period)
                out[lr, :, g] = (period_excess(period, peak, rest, strength, min_strength), peak, rest, strength, period, ago, n)
    return out


class _OraclePeriods:
    def __init__(self, periods, scores, first_rank, n_ranks):
        self._rec = (periods, scores)
        self.first_rank, self.n_ranks = first_rank, n_ranks
        self.reads = 0

    def records(self):
        self.reads += 1
        return self._rec


class _PeriodRingsMixin:
    def period_local(self, ws, max_period, min_strength, rows_active=0, fused=False):
        assert self.onset_enabled, "period_local() before onset_enable(): no ring-start snapshot"
        self.backend.period_local_calls += 1
        KS = ws.K + ws.S
        if getattr(ws, "_period_table", None) is None:
            ws._period_table = torch.zeros((ws.R, PLANES * KS), dtype=torch.float32)
            ws._period_send = ws._period_table if ws.R == ws.local_ranks else torch.zeros((ws.local_ranks, PLANES * KS), dtype=torch.float32)
        planes = ring_periods(self, ws.K, ws.S, max_period, min_strength, rows_active)
        ws._period_send.copy_(torch.from_numpy(planes.reshape(self.local_ranks, PLANES * KS)))
        return ws._period_send, ws._period_table


class PeriodOracleRings(_PeriodRingsMixin, _OnsetRingsMixin, _TailRingsMixin, OracleRings):
    pass


class PeriodOracleRingsFused(_PeriodRingsMixin, _OnsetRingsMixin, _TailRingsMixin, OracleRingsFused):
    pass


class PeriodOracleBackend(OnsetOracleBackend):
    """The CPU checker with period scores (computed at enqueue time, like its scores) -- and tail and onset scores, for the
    reports that carry several."""

    name = "oracle-test+periods"

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.period_local_calls = 0
        self.period_score_calls = 0
        self.period_handles = []

    def make_rings(self, local_ranks, rows_per_rank, ring_cap):
        cls = PeriodOracleRingsFused if self.emulate_fused else PeriodOracleRings
        return cls(self, local_ranks, rows_per_rank, ring_cap)

    def period_score(self, ws, periods, table, first_rank=0, n_ranks=None):
        self.period_score_calls += 1
        n_ranks = ws.R - first_rank if n_ranks is None else n_ranks
        O = periods.numpy().copy().reshape(ws.R, PLANES, ws.K + ws.S)
        sc = period_scores_table(O, table.numpy().copy(), ws.K, ws.S, first_rank, n_ranks)
        h = _OraclePeriods(O[first_rank : first_rank + n_ranks], sc, first_rank, n_ranks)
        self.period_handles.append(h)
        return h


class _SpyRings(OracleRings):
    def _spied(self, *a, **kw):
        self.backend.period_calls += 1
        raise AssertionError("a period method of the rings was called although period_detection is off")

    onset_enable = period_local = _spied


class _SpyRingsFused(OracleRingsFused):
    onset_enable = period_local = _SpyRings._spied


class SpyPeriodBackend(OracleBackend):
    """The plain checker plus period methods that only count and raise: with the option off nobody may call them (the
    ring-start snapshot included)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.period_calls = 0

    def make_rings(self, local_ranks, rows_per_rank, ring_cap):
        cls = _SpyRingsFused if self.emulate_fused else _SpyRings
        return cls(self, local_ranks, rows_per_rank, ring_cap)

    def period_score(self, *a, **kw):
        self.period_calls += 1
        raise AssertionError("period_score() called although period_detection is off")
