"""Onset scores for the CPU checker backend, and the NumPy restatement the onset tests compare against -- TEST
INFRASTRUCTURE, lives outside the product.

``row_onset`` / ``onset_shift`` / ``onset_scores_table`` restate the definitions of include/nvrx_straggler.h
(``nvrx_row_onset``, ``nvrx_onset_score``) in NumPy: float64 ``cumsum`` over the samples in time order, pivoted on the first
one.  ``OnsetOracleBackend`` / ``OnsetOracleRings`` are ``TailOracleBackend`` / ``TailOracleRings`` plus ``onset_enable`` /
``onset_local`` / ``onset_score`` built on them, so that the host side of the feature (option plumbing, collectives, names,
lifetime, pickling) runs on a box without a GPU.
"""
import numpy as np
import torch

from oracle_backend import OracleBackend, OracleRings, OracleRingsFused
from tail_oracle_backend import TailOracleBackend, _TailRingsMixin, tail_scores_table

NAN32 = np.float32(np.nan)
PLANES = 6  # {e, before, after, strength, ago, n}


def min_segment(seg_ppm, n):
    """max(8, ceil(seg_ppm * n / 1e6)), the exact rational."""
    return max(8, -(-int(seg_ppm) * int(n) // 10**6))


def time_order(x, n, start=0):
    """The row's n valid samples, oldest first: sample i lives in slot (start + i) mod n."""
    x = np.asarray(x, dtype=np.float32)[:n]
    start = int(start) % n
    return np.concatenate([x[start:], x[:start]])


def split_curve(x):
    """``(t, D_t, before_t, after_t, SST, T)`` of a row in time order for every t in [1, n - 1], in float64 over values
    pivoted on the first sample (the means are the pivoted ones)."""
    d = x.astype(np.float64) - np.float64(x[0])
    n = d.size
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.cumsum(d)
        T = c[-1]
        t = np.arange(1, n, dtype=np.float64)
        before = c[:-1] / t
        after = (T - c[:-1]) / (n - t)
        D = t * (n - t) / n * (after - before) ** 2
        sst = ((d - T / n) ** 2).sum()
    return t, D, before, after, sst, T


def row_onset_one(x, seg_ppm):
    """``(ago, before, after, strength)`` of one row given in time order (n >= 1), and the curve ``strength_t`` over the
    admissible splits ``[m, n - m]`` (None where there is none)."""
    n = x.size
    m = min_segment(seg_ppm, n)
    t, D, before, after, sst, T = split_curve(x)
    if not (np.isfinite(T) and np.isfinite(sst)):
        return (0, NAN32, NAN32, NAN32), None
    if n < 2 * m:
        mean = np.float32(np.float64(x[0]) + T / n)
        return (0, mean, mean, np.float32(0.0)), None
    if sst == 0.0:
        return (n - m, np.float32(x[0]), np.float32(x[0]), np.float32(0.0)), None
    lo, hi = m - 1, n - m  # indices of t = m .. n - m in the arrays that start at t = 1
    k = lo + int(np.argmax(D[lo:hi]))  # (the first of equals)
    ts = k + 1
    rec = (n - ts, np.float32(np.float64(x[0]) + before[k]), np.float32(np.float64(x[0]) + after[k]), np.float32(D[k] / sst))
    return rec, D[lo:hi] / sst


def row_onset(samples, counts, seg_ppm, starts=None):
    """``[rows]`` structured records ``{ago u32, before, after, strength f32}`` of every row (absent: {0, -1, -1, -1}), and
    per row the strength curve over its admissible splits (or None)."""
    samples = np.asarray(samples, dtype=np.float32)
    rows = samples.shape[0]
    out = np.zeros(rows, dtype=[("ago", np.uint32), ("before", np.float32), ("after", np.float32), ("strength", np.float32)])
    curves = []
    for r, n in enumerate(np.asarray(counts).tolist()):
        n = min(int(n), samples.shape[1])
        if n == 0:
            out[r] = (0, -1.0, -1.0, -1.0)
            curves.append(None)
            continue
        rec, curve = row_onset_one(time_order(samples[r], n, 0 if starts is None else starts[r]), seg_ppm)
        out[r] = rec
        curves.append(curve)
    return out, curves


def onset_shift(before, after, strength, min_strength):
    """The effective shift of a record: f32 of the f64 quotient after / before where the step is a convincing slow-down."""
    before, after, strength = np.float32(before), np.float32(after), np.float32(strength)
    with np.errstate(invalid="ignore"):
        if strength >= np.float32(min_strength) and after > before and before > 0:
            return np.float32(np.float64(after) / np.float64(before))
    return np.float32(1.0)


def onset_scores_table(onsets, table, K, S, first_rank=0, n_ranks=None):
    """``[n_ranks, 1 + S]`` f32 {GPU onset score, section onset scores} from the onset table ``onsets`` [R, 6, K+S] (plane 0:
    the effective shifts) and the weights in the exchange table ``table`` [R, L]: the tail scores' arithmetic on plane 0."""
    onsets = np.asarray(onsets, dtype=np.float32)
    return tail_scores_table(np.ascontiguousarray(onsets[:, 0, :]), table, K, S, first_rank, n_ranks)


def ring_onsets(rings, ws_K, ws_S, seg_ppm, min_strength, rows_active=0):
    """[local_ranks, 6, K+S] onset planes of NumPy rings (``OracleRings``), packed by gid."""
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
                (ago, before, after, strength), _ = row_onset_one(time_order(rings.samples[r], n, start), seg_ppm)
                out[lr, :, g] = (onset_shift(before, after, strength, min_strength), before, after, strength, ago, n)
    return out


class _OracleOnsets:
    def __init__(self, onsets, scores, first_rank, n_ranks):
        self._rec = (onsets, scores)
        self.first_rank, self.n_ranks = first_rank, n_ranks
        self.reads = 0

    def records(self):
        self.reads += 1
        return self._rec


class _OnsetRingsMixin:
    onset_enabled = False

    def onset_enable(self, on=True):
        self.backend.onset_enable_calls += 1
        self.onset_enabled = bool(on)

    def onset_local(self, ws, seg_ppm, min_strength, rows_active=0, fused=False):
        assert self.onset_enabled, "onset_local() before onset_enable()"
        self.backend.onset_local_calls += 1
        KS = ws.K + ws.S
        if getattr(ws, "_onset_table", None) is None:
            ws._onset_table = torch.zeros((ws.R, PLANES * KS), dtype=torch.float32)
            ws._onset_send = ws._onset_table if ws.R == ws.local_ranks else torch.zeros((ws.local_ranks, PLANES * KS), dtype=torch.float32)
        planes = ring_onsets(self, ws.K, ws.S, seg_ppm, min_strength, rows_active)
        ws._onset_send.copy_(torch.from_numpy(planes.reshape(self.local_ranks, PLANES * KS)))
        return ws._onset_send, ws._onset_table


class OnsetOracleRings(_OnsetRingsMixin, _TailRingsMixin, OracleRings):
    pass


class OnsetOracleRingsFused(_OnsetRingsMixin, _TailRingsMixin, OracleRingsFused):
    pass


class OnsetOracleBackend(TailOracleBackend):
    """The CPU checker with onset scores (computed at enqueue time, like its scores) -- and tail scores, for the reports that
    carry both."""

    name = "oracle-test+onsets"

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.onset_enable_calls = 0
        self.onset_local_calls = 0
        self.onset_score_calls = 0
        self.onset_handles = []

    def make_rings(self, local_ranks, rows_per_rank, ring_cap):
        cls = OnsetOracleRingsFused if self.emulate_fused else OnsetOracleRings
        return cls(self, local_ranks, rows_per_rank, ring_cap)

    def onset_score(self, ws, onsets, table, first_rank=0, n_ranks=None):
        self.onset_score_calls += 1
        n_ranks = ws.R - first_rank if n_ranks is None else n_ranks
        O = onsets.numpy().copy().reshape(ws.R, PLANES, ws.K + ws.S)
        sc = onset_scores_table(O, table.numpy().copy(), ws.K, ws.S, first_rank, n_ranks)
        h = _OracleOnsets(O[first_rank : first_rank + n_ranks], sc, first_rank, n_ranks)
        self.onset_handles.append(h)
        return h


class _SpyRings(OracleRings):
    def _spied(self, *a, **kw):
        self.backend.onset_calls += 1
        raise AssertionError("an onset method of the rings was called although onset_detection is off")

    onset_enable = onset_local = _spied


class _SpyRingsFused(OracleRingsFused):
    onset_enable = onset_local = _SpyRings._spied


class SpyOnsetBackend(OracleBackend):
    """The plain checker plus onset methods that only count and raise: with the option off nobody may call them."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.onset_calls = 0

    def make_rings(self, local_ranks, rows_per_rank, ring_cap):
        cls = _SpyRingsFused if self.emulate_fused else _SpyRings
        return cls(self, local_ranks, rows_per_rank, ring_cap)

    def onset_score(self, *a, **kw):
        self.onset_calls += 1
        raise AssertionError("onset_score() called although onset_detection is off")
