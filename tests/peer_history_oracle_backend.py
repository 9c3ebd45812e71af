"""The peer-score history and trends for the CPU checker backend, and the restatement the peer-history tests compare against
-- TEST INFRASTRUCTURE, lives outside the product.

The contract of include/nvrx_straggler.h (``nvrx_peer_history`` / ``nvrx_peer_trend``) is stated by reference: the record of
cell (r, j) is the record ``nvrx_score_history`` / ``nvrx_score_trend`` write for (r, f = 1, j) on score rows whose relative
columns hold the peer values.  So ``peer_history_step`` / ``peer_trend_records`` place the peer plane there and call the
existing restatements (``history_oracle_backend.history_step``, ``trend_oracle_backend.trend_records``) -- imported, not
copied -- and take family 1.  ``PeerHistoryOracleBackend`` / its rings are the checker with everything a report can carry
(``WorkOracleBackend``) plus ``peer_history`` / ``peer_trend`` and their ``report_`` forms, so that the host side of the
feature runs on a box without a GPU.  ``CountingPeerHistoryBackend`` has those methods only count and raise: with the option
off nobody may call them.
"""
import numpy as np

from history_oracle_backend import history_step, stride
from trend_oracle_backend import trend_records
from work_oracle_backend import WorkOracleBackend, WorkOracleRings, WorkOracleRingsFused


def peer_fresh(n_ranks, S_cap, H):
    """A peer ring nothing was appended to: f32 ``[n_ranks, 1 + S_cap, stride(H)]``, bytes 0xFF."""
    return np.full((n_ranks, 1 + S_cap, stride(H)), 0xFFFFFFFF, dtype=np.uint32).view(np.float32)


def embed(peer, S):
    """The peer plane ``[n, 1 + S]`` f32 as score rows ``[n, 2 + 2S]``: the relative columns (1, and 2 + S + s) hold the peer
    values bit for bit, the individual ones a NaN."""
    peer = np.ascontiguousarray(peer, dtype=np.float32)
    rows = np.full((peer.shape[0], 2 + 2 * S), 0xFFFFFFFF, dtype=np.uint32)
    rows[:, 1] = peer.view(np.uint32)[:, 0]
    rows[:, 2 + S :] = peer.view(np.uint32)[:, 1:]
    return rows.view(np.float32)


def as_score_ring(hist):
    """The peer ring ``[n, 1 + S_cap, Hs]`` as family 1 of a score-history ring ``[n, 2, 1 + S_cap, Hs]`` (family 0 fresh)."""
    ring = np.full((hist.shape[0], 2) + hist.shape[1:], 0xFFFFFFFF, dtype=np.uint32)
    ring[:, 1] = hist.view(np.uint32)
    return ring.view(np.float32)


def peer_history_step(hist, peer, S, H, n_before, thresholds=None):
    """Append one report's peer plane (``peer`` [n_ranks, 1 + S] f32) to ``hist`` (f32 ``[n_ranks, 1 + S_cap, stride(H)]``,
    changed in place) and return the records ``[n_ranks, 1, 1 + S, 8]`` uint32: ``history_step`` on the embedded rows,
    family 1, with ``(gpu, section)`` thresholds."""
    n = hist.shape[0]
    thr = (0.75, 0.75) if thresholds is None else tuple(float(t) for t in thresholds)
    ring = as_score_ring(hist)
    rec = history_step(ring, embed(peer, S), S, 0, n, H, n_before, (thr[0], thr[1], 0.75, 0.75))
    hist.view(np.uint32)[...] = ring.view(np.uint32)[:, 1]
    return rec[:, 1:2].copy()


def peer_trend_records(hist, S, H, n_reports):
    """``[n_ranks, 1, 1 + S, 4]`` uint32 of the peer ring after ``n_reports`` appended reports: ``trend_records``, family 1."""
    return trend_records(as_score_ring(hist), S, H, n_reports)[:, 1:2].copy()


class _OracleRecords:
    def __init__(self, rec, first_rank=0, n_ranks=None):
        self._rec = rec
        self.first_rank, self.n_ranks = first_rank, rec.shape[0] if n_ranks is None else n_ranks
        self.reads = 0

    def records(self):
        self.reads += 1
        return self._rec


def _peer_history(backend, ws, state, peer, thresholds):
    """The product's step (backend.HipBackend._peer_history_step) on the checker's peer handle: same restart, same growth."""
    backend.peer_history_calls += 1
    first_rank, n_ranks = peer.first_rank, peer.n_ranks
    state.begin(first_rank, n_ranks)
    if state.hist is None or ws.S > state.S_cap:
        cap = state.capacity(ws.S)
        ring = peer_fresh(n_ranks, cap, state.depth)
        if state.hist is not None:
            ring[:, : 1 + state.S_cap] = state.hist
            backend.peer_history_grown += 1
        state.hist, state.S_cap = ring, cap
    thr = tuple(float(t) for t in thresholds)
    assert len(thr) == 2, thr
    backend.peer_history_args.append((first_rank, n_ranks, ws.S, state.n_before, thr))
    scores = peer._rec[1]  # (the rank part of the peer step's block, where that step left it: not a read of the handle)
    assert scores.shape == (n_ranks, 1 + ws.S), (scores.shape, n_ranks, ws.S)
    rec = peer_history_step(state.hist, scores, ws.S, state.depth, state.n_before, thr)
    state.n_before += 1
    h = _OracleRecords(rec, first_rank, n_ranks)
    backend.peer_history_handles.append(h)
    return h


def _peer_trend(backend, ws, state):
    backend.peer_trend_calls += 1
    backend.peer_trend_args.append((state.ranks, ws.S, state.n_before))
    t = _OracleRecords(peer_trend_records(state.hist, ws.S, state.depth, state.n_before))
    backend.peer_trend_handles.append(t)
    return t


class _PeerHistoryRingsMixin:
    def report_peer_history(self, ws, state, peer, thresholds=(0.75, 0.75)):
        return _peer_history(self.backend, ws, state, peer, thresholds)

    def report_peer_trend(self, ws, state):
        return _peer_trend(self.backend, ws, state)


class PeerHistoryOracleRings(_PeerHistoryRingsMixin, WorkOracleRings):
    pass


class PeerHistoryOracleRingsFused(_PeerHistoryRingsMixin, WorkOracleRingsFused):
    pass


class PeerHistoryOracleBackend(WorkOracleBackend):
    """The CPU checker with everything a report can carry, the peer-score history and trends included (computed at enqueue
    time)."""

    name = "oracle-test+peer-history"

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.peer_history_calls = self.peer_history_grown = self.peer_trend_calls = 0
        self.peer_history_args, self.peer_history_handles = [], []
        self.peer_trend_args, self.peer_trend_handles = [], []

    def make_rings(self, local_ranks, rows_per_rank, ring_cap):
        cls = PeerHistoryOracleRingsFused if self.emulate_fused else PeerHistoryOracleRings
        return cls(self, local_ranks, rows_per_rank, ring_cap)

    def peer_history(self, ws, state, peer, thresholds=(0.75, 0.75)):
        return _peer_history(self, ws, state, peer, thresholds)

    def peer_trend(self, ws, state):
        return _peer_trend(self, ws, state)


class _RaisingMixin:
    def report_peer_history(self, *a, **kw):
        self.backend.peer_history_calls += 1
        raise AssertionError("report_peer_history() called although peer_history is off")

    def report_peer_trend(self, *a, **kw):
        self.backend.peer_history_calls += 1
        raise AssertionError("report_peer_trend() called although peer_trends is off")


class _RaisingRings(_RaisingMixin, WorkOracleRings):
    pass


class _RaisingRingsFused(_RaisingMixin, WorkOracleRingsFused):
    pass


class CountingPeerHistoryBackend(WorkOracleBackend):
    """The checker with everything else working -- peer scores included -- and peer-history methods that only count and
    raise."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.peer_history_calls = 0

    def make_rings(self, local_ranks, rows_per_rank, ring_cap):
        cls = _RaisingRingsFused if self.emulate_fused else _RaisingRings
        return cls(self, local_ranks, rows_per_rank, ring_cap)

    def peer_history(self, *a, **kw):
        self.peer_history_calls += 1
        raise AssertionError("peer_history() called although peer_history is off")

    def peer_trend(self, *a, **kw):
        self.peer_history_calls += 1
        raise AssertionError("peer_trend() called although peer_trends is off")
