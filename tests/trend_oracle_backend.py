"""Score trends for the CPU checker backend, and the NumPy restatement the trend tests compare against -- TEST INFRASTRUCTURE,
lives outside the product.

``trend_records`` restates the contract of include/nvrx_straggler.h (``nvrx_score_trend``) in NumPy by brute force: it forms
every pair slope with the header's f64 expression, SORTS them by key and takes the element of rank ``(N - 1) >> 1`` -- no
bisection, no counting: the selection shares nothing with the kernel's.  ``TrendOracleBackend`` / its rings are the checker
with everything a report can carry (``HistoryOracleBackend``) plus ``score_trend`` / ``report_trend`` built on it, so that
the host side of the feature runs on a box without a GPU.  ``CountingTrendBackend`` keeps the history and has trend methods
that only count and raise: with the option off nobody may call them.
"""
import numpy as np

from history_oracle_backend import HistoryOracleBackend, HistoryOracleRings, HistoryOracleRingsFused, stride
from tail_oracle_backend import f2key, key2f

NAN_BITS = np.uint32(0x7FC00000)
ABSENT = np.uint32(0xFFFFFFFF)
RECORD = ("slope", "level", "S", "usable")


def aged(hist, S, H, n_reports):
    """``[n_ranks, 2, 1 + S, depth]`` f32: the entries of every cell, newest first (age a at position (n_reports - 1 - a) % H)."""
    assert n_reports >= 1 and hist.dtype == np.float32 and hist.shape[3] == stride(H) and S <= hist.shape[2] - 1
    depth = min(n_reports, H)
    at = (n_reports - 1 - np.arange(depth)) % H
    return np.ascontiguousarray(hist[:, :, : 1 + S, :][..., at])


def pair_slopes(x, chunk=256):
    """``x`` [..., depth] f32, newest first -> (keys [..., P] uint32 of the slopes of all P pairs of ages a < b, ABSENT where a
    pair has an entry that is not finite; the number of pairs that exist [...]; the sum of sign(x_a - x_b) over them [...]).
    (Worked ``chunk`` cells at a time with the pairs on the leading axis: gathers of whole rows, temporaries that fit a cache.)"""
    depth, cells = x.shape[-1], x.shape[:-1]
    a, b = np.triu_indices(depth, 1)
    by = (b - a).astype(np.float64)[:, None]
    flat = x.reshape(-1, depth)
    keys = np.empty((flat.shape[0], a.size), dtype=np.uint32)
    n_valid, sign = np.empty(flat.shape[0], dtype=np.int64), np.empty(flat.shape[0], dtype=np.int64)
    for lo in range(0, flat.shape[0], chunk):
        xt = np.ascontiguousarray(flat[lo : lo + chunk].T).astype(np.float64)  # [depth, cells]; f32 -> f64 is exact
        ok = np.isfinite(xt)
        valid = ok[a] & ok[b]
        with np.errstate(invalid="ignore", over="ignore"):
            d = xt[a] - xt[b]                              # (double)x_a - (double)x_b: its sign is that of the f32 comparison
            sign[lo : lo + chunk] = np.where(valid, np.sign(d), 0.0).sum(0)
            d /= by
            slope = d.astype(np.float32)
        keys[lo : lo + chunk] = np.where(valid, f2key(slope), ABSENT).T
        n_valid[lo : lo + chunk] = valid.sum(0)
    return keys.reshape(cells + (a.size,)), n_valid.reshape(cells), sign.reshape(cells)


def _ranked(keys, k, n):
    """The bits of the element of rank ``k`` of every row of ``keys`` sorted; NaN where ``n`` is 0."""
    keys = np.sort(keys, axis=-1)
    if keys.shape[-1] == 0:
        return np.full(k.shape, NAN_BITS, dtype=np.uint32)
    picked = np.take_along_axis(keys, np.clip(k, 0, keys.shape[-1] - 1)[..., None], axis=-1)[..., 0]
    return np.where(n > 0, key2f(picked).view(np.uint32), NAN_BITS)


def trend_records(hist, S, H, n_reports):
    """``[n_ranks, 2, 1 + S, 4]`` uint32 ``{slope, level, S, usable}`` of the ring ``hist`` (f32 ``[n_ranks, 2, 1 + S_cap,
    stride(H)]``) after ``n_reports`` appended reports."""
    x = aged(hist, S, H, n_reports)
    depth = x.shape[-1]
    usable = np.isfinite(x)
    p = usable.sum(-1).astype(np.int64)
    keys, n_valid, sign = pair_slopes(x)
    n_pairs = p * (p - 1) // 2
    assert np.array_equal(n_valid, n_pairs)
    slope_bits = _ranked(keys, (n_pairs - 1) >> 1, n_pairs)
    slope = slope_bits.view(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        moved = (x.astype(np.float64) + slope.astype(np.float64)[..., None] * np.arange(depth, dtype=np.float64)).astype(np.float32)
    v = np.where((p >= 2)[..., None], moved, x)
    v = np.where(np.isnan(v), NAN_BITS.view(np.float32), v).astype(np.float32)  # (a NaN v_a counts as 0x7FC00000)
    level_bits = _ranked(np.where(usable, f2key(v), ABSENT), (p - 1) >> 1, p)
    out = np.empty(x.shape[:-1] + (4,), dtype=np.uint32)
    out[..., 0] = slope_bits
    out[..., 1] = level_bits
    out[..., 2] = sign.astype(np.int32).view(np.uint32)
    out[..., 3] = p
    return out


def as_dict(rec):
    """One record (4 uint32 words) with its words named."""
    rec = np.ascontiguousarray(rec, dtype=np.uint32)
    f = rec[:2].view(np.float32).tolist()
    return {"slope": f[0], "level": f[1], "S": int(rec[2:3].view(np.int32)[0]), "usable": int(rec[3])}


class _OracleTrend:
    def __init__(self, rec):
        self._rec = rec
        self.reads = 0

    def records(self):
        self.reads += 1
        return self._rec


def _trend(backend, ws, state):
    backend.trend_calls += 1
    backend.trend_args.append((state.ranks, ws.S, state.n_before))
    t = _OracleTrend(trend_records(state.hist, ws.S, state.depth, state.n_before))
    backend.trend_handles.append(t)
    return t


class _TrendRingsMixin:
    def report_trend(self, ws, state):
        return _trend(self.backend, ws, state)


class TrendOracleRings(_TrendRingsMixin, HistoryOracleRings):
    pass


class TrendOracleRingsFused(_TrendRingsMixin, HistoryOracleRingsFused):
    pass


class TrendOracleBackend(HistoryOracleBackend):
    """The CPU checker with everything a report can carry, score trends included (computed at enqueue time)."""

    name = "oracle-test+trend"

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.trend_calls = 0
        self.trend_args = []
        self.trend_handles = []

    def make_rings(self, local_ranks, rows_per_rank, ring_cap):
        cls = TrendOracleRingsFused if self.emulate_fused else TrendOracleRings
        return cls(self, local_ranks, rows_per_rank, ring_cap)

    def score_trend(self, ws, state):
        return _trend(self, ws, state)


class _RaisingTrendRings(HistoryOracleRings):
    def report_trend(self, *a, **kw):
        self.backend.trend_calls += 1
        raise AssertionError("report_trend() called although score_trends is off")


class _RaisingTrendRingsFused(HistoryOracleRingsFused):
    report_trend = _RaisingTrendRings.report_trend


class CountingTrendBackend(HistoryOracleBackend):
    """The checker with a working score history and trend methods that only count and raise."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.trend_calls = 0

    def make_rings(self, local_ranks, rows_per_rank, ring_cap):
        cls = _RaisingTrendRingsFused if self.emulate_fused else _RaisingTrendRings
        return cls(self, local_ranks, rows_per_rank, ring_cap)

    def score_trend(self, *a, **kw):
        self.trend_calls += 1
        raise AssertionError("score_trend() called although score_trends is off")
