"""The score history for the CPU checker backend, and the NumPy restatement the history tests compare against -- TEST
INFRASTRUCTURE, lives outside the product.

``history_step`` restates the contract of include/nvrx_straggler.h (``nvrx_score_history``) in NumPy: it appends one report's
scores to the ring and returns the records, with a sort where the kernel counts.  ``HistoryOracleBackend`` / its rings are the
checker with every row family (``EpisodeOracleBackend``) plus kernel attribution and robust scores (``RobustOracleBackend``'s)
plus ``score_history`` / ``report_history`` built on ``history_step``, so that the host side of the feature (option plumbing,
growth, restart, lifetime, pickling, all the follow-ups together) runs on a box without a GPU.
"""
import numpy as np

from attribution_oracle_backend import AttributionOracleBackend
from episode_oracle_backend import EpisodeOracleBackend, EpisodeOracleRings, EpisodeOracleRingsFused
from oracle_backend import OracleBackend, OracleRings, OracleRingsFused
from robust_oracle_backend import RobustOracleBackend, _RobustRingsMixin
from tail_oracle_backend import f2key, key2f

NAN_BITS = np.uint32(0x7FC00000)
MAX_DEPTH = 64
RECORD = ("latest", "median", "worst", "best", "streak", "below", "present", "depth")


def stride(H):
    """NVRX_HISTORY_STRIDE."""
    return 16 if H <= 16 else 32 if H <= 32 else 64


def fresh(n_ranks, S_cap, H):
    """A ring nothing was appended to: f32 ``[n_ranks, 2, 1 + S_cap, stride(H)]``, bytes 0xFF."""
    return np.full((n_ranks, 2, 1 + S_cap, stride(H)), 0xFFFFFFFF, dtype=np.uint32).view(np.float32)


def columns(S):
    """``[2, 1 + S]``: the column of the score row that (family, slot) reads."""
    col = np.empty((2, 1 + S), dtype=np.int64)
    col[:, 0] = (0, 1)
    col[0, 1:] = 2 + np.arange(S)
    col[1, 1:] = 2 + S + np.arange(S)
    return col


def threshold_table(S, thresholds=None):
    """``[2, 1 + S]`` f64: nvrx_score's {gpu_rel, section_rel, gpu_indiv, section_indiv} per (family, slot)."""
    t = (0.75,) * 4 if thresholds is None else tuple(float(x) for x in thresholds)
    thr = np.empty((2, 1 + S), dtype=np.float64)
    thr[1, 0], thr[1, 1:], thr[0, 0], thr[0, 1:] = t[0], t[1], t[2], t[3]
    return thr


def history_step(hist, scores, S, first_rank, n_ranks, H, n_before, thresholds=None):
    """Append the scores of one report (``scores`` [R, 2 + 2S] f32) to ``hist`` (f32 ``[n_ranks, 2, 1 + S_cap, stride(H)]``,
    changed in place: position ``n_before % H`` of every slot j <= S) and return the records ``[n_ranks, 2, 1 + S, 8]``
    uint32 ``{latest, median, worst, best, streak, below, present, depth}``."""
    assert 2 <= H <= MAX_DEPTH and hist.dtype == np.float32 and hist.shape[0] == n_ranks and hist.shape[3] == stride(H)
    assert S <= hist.shape[2] - 1
    bits = hist.view(np.uint32)
    rows = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32)[first_rank : first_rank + n_ranks]
    bits[:, :, : 1 + S, n_before % H] = rows[:, columns(S)]
    depth = min(n_before + 1, H)
    at = (n_before - np.arange(depth)) % H                      # position of the entry of age a
    aged = bits[:, :, : 1 + S, :][..., at]                      # [n_ranks, 2, 1 + S, depth], newest first
    x = aged.view(np.float32)
    present = ~np.isnan(x)
    with np.errstate(invalid="ignore"):
        below = x.astype(np.float64) < threshold_table(S, thresholds)[None, :, :, None]
    n_present = present.sum(-1)
    keys = np.sort(np.where(present, f2key(x), np.uint32(0xFFFFFFFF)), axis=-1)  # (absent entries order behind +inf)

    def ranked(k):
        picked = np.take_along_axis(keys, np.clip(k, 0, depth - 1)[..., None], axis=-1)[..., 0]
        return np.where(n_present > 0, key2f(picked).view(np.uint32), NAN_BITS)

    out = np.empty((n_ranks, 2, 1 + S, 8), dtype=np.uint32)
    out[..., 0] = aged[..., 0]
    out[..., 1] = ranked((n_present - 1) >> 1)
    out[..., 2] = ranked(np.zeros_like(n_present))
    out[..., 3] = ranked(n_present - 1)
    out[..., 4] = np.cumprod(below, axis=-1).sum(-1)            # newest entries that are ALL below
    out[..., 5] = below.sum(-1)
    out[..., 6] = n_present
    out[..., 7] = depth
    return out


def as_dicts(rec):
    """One record (8 uint32 words) as ``Report.score_history()`` shows it."""
    f = np.ascontiguousarray(rec[:4]).view(np.float32).tolist()
    return {"latest": f[0], "median": f[1], "worst": f[2], "best": f[3], "streak": int(rec[4]), "below": int(rec[5]),
            "present": int(rec[6])}


class _OracleHistory:
    def __init__(self, rec, first_rank, n_ranks):
        self._rec = rec
        self.first_rank, self.n_ranks = first_rank, n_ranks
        self.reads = 0

    def records(self):
        self.reads += 1
        return self._rec


def _history(backend, ws, state, first_rank, n_ranks, thresholds):
    """The product's step (backend.HipBackend.score_history) on the checker's host block: same restart, same growth."""
    backend.history_calls += 1
    n_ranks = ws.R - first_rank if n_ranks is None else n_ranks
    state.begin(first_rank, n_ranks)
    if state.hist is None or ws.S > state.S_cap:
        cap = state.capacity(ws.S)
        ring = fresh(n_ranks, cap, state.depth)
        if state.hist is not None:
            ring[:, :, : 1 + state.S_cap] = state.hist
            backend.history_grown += 1
        state.hist, state.S_cap = ring, cap
    backend.history_args.append((first_rank, n_ranks, ws.S, state.n_before, tuple(thresholds)))
    rec = history_step(state.hist, ws.scores, ws.S, first_rank, n_ranks, state.depth, state.n_before, thresholds)
    state.n_before += 1
    h = _OracleHistory(rec, first_rank, n_ranks)
    backend.history_handles.append(h)
    return h


class _HistoryRingsMixin:
    def report_history(self, ws, state, first_rank=0, n_ranks=None, thresholds=(0.75,) * 4):
        return _history(self.backend, ws, state, first_rank, n_ranks, thresholds)


class HistoryOracleRings(_HistoryRingsMixin, EpisodeOracleRings):
    pass


class HistoryOracleRingsFused(_HistoryRingsMixin, _RobustRingsMixin, EpisodeOracleRingsFused):
    pass


class HistoryOracleBackend(EpisodeOracleBackend):
    """The CPU checker with everything a report can carry: the four row families, kernel attribution, robust scores and the
    score history (computed at enqueue time, like its scores)."""

    name = "oracle-test+history"

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.attribute_calls = 0
        self.robust_calls = 0
        self.robust_args = []
        self.robust_handles = []
        self.history_calls = 0
        self.history_grown = 0
        self.history_args = []
        self.history_handles = []

    attribute = AttributionOracleBackend.attribute
    robust_score = RobustOracleBackend.robust_score

    def make_rings(self, local_ranks, rows_per_rank, ring_cap):
        cls = HistoryOracleRingsFused if self.emulate_fused else HistoryOracleRings
        return cls(self, local_ranks, rows_per_rank, ring_cap)

    def score_history(self, ws, state, first_rank=0, n_ranks=None, thresholds=(0.75,) * 4):
        return _history(self, ws, state, first_rank, n_ranks, thresholds)


class _RaisingRings(OracleRings):
    def report_history(self, *a, **kw):
        self.backend.history_calls += 1
        raise AssertionError("report_history() called although score_history is off")


class _RaisingRingsFused(OracleRingsFused):
    report_history = _RaisingRings.report_history


class CountingHistoryBackend(OracleBackend):
    """The plain checker plus ``score_history`` / ``report_history`` that only count and raise: with the option off nobody
    may call them."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.history_calls = 0

    def make_rings(self, local_ranks, rows_per_rank, ring_cap):
        cls = _RaisingRingsFused if self.emulate_fused else _RaisingRings
        return cls(self, local_ranks, rows_per_rank, ring_cap)

    def score_history(self, *a, **kw):
        self.history_calls += 1
        raise AssertionError("score_history() called although score_history is off")
