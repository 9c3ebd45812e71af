"""Tail scores for the CPU checker backend, and the NumPy restatement the tail tests compare against -- TEST INFRASTRUCTURE,
lives outside the product.

``row_quantile`` / ``tail_scores_table`` restate the definitions of include/nvrx_straggler.h (``nvrx_row_quantile``,
``nvrx_tail_score``) in NumPy; ``TailOracleBackend`` / ``TailOracleRings`` are ``OracleBackend`` / ``OracleRings`` plus
``tail_local`` / ``tail_score`` built on them, so that the host side of the feature (option plumbing, collectives, names,
lifetime, pickling) runs on a box without a GPU.
"""
import numpy as np
import torch

from oracle_backend import OracleBackend, OracleRings, OracleRingsFused

NAN32 = np.float32(np.nan)


def tail_rank(q_ppm, n):
    """The exact rational ceil(q_ppm * n / 1e6) - 1."""
    return -(-int(q_ppm) * int(n) // 10**6) - 1


def f2key(x):
    """Order-preserving map of f32 bit patterns to uint32 (-inf < negatives < -0.0 < +0.0 < positives < +inf < NaN)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u >> 31, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key2f(k):
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k >> 31, k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def row_quantile(samples, counts, q_ppm):
    """[rows] f32: the element of rank ``tail_rank(q_ppm, n)`` of every row's first n samples sorted by key; -1 where n == 0."""
    samples = np.asarray(samples, dtype=np.float32)
    out = np.full(samples.shape[0], -1.0, dtype=np.float32)
    for r, n in enumerate(np.asarray(counts).tolist()):
        n = min(int(n), samples.shape[1])
        if n > 0:
            keys = np.sort(f2key(samples[r, :n]))
            out[r] = key2f(keys[tail_rank(q_ppm, n)])
    return out


def tail_scores_table(tails, table, K, S, first_rank=0, n_ranks=None):
    """``[n_ranks, 1 + S]`` f32 {GPU tail score, section tail scores} from the tail table ``tails`` [R, K+S] and the weights
    in the exchange table ``table`` [R, L]."""
    tails = np.asarray(tails, dtype=np.float32)
    table = np.asarray(table, dtype=np.float32)
    R, KS = tails.shape[0], K + S
    n_ranks = R - first_rank if n_ranks is None else n_ranks
    with np.errstate(invalid="ignore"):
        m = np.full(KS, np.inf, dtype=np.float32)
        for r in range(R):  # the rule of k_colmin: v < m, NaN never wins
            m = np.where(tails[r] < m, tails[r], m)
        ref = np.where(m >= 0, m, NAN32).astype(np.float32)
    out = np.full((n_ranks, 1 + S), NAN32, dtype=np.float32)
    for i in range(n_ranks):
        r = first_rank + i
        t = tails[r]
        with np.errstate(invalid="ignore", divide="ignore"):
            have = t[K:] >= 0
            quot = ref[K:].astype(np.float64) / t[K:].astype(np.float64)
            out[i, 1:] = np.where(have, quot, np.nan).astype(np.float32)
            elig = (t[:K] >= 0) & ~np.isnan(ref[:K])
            if elig.any():
                w = table[r, 2 * KS : 2 * KS + K].astype(np.float64)[elig]
                s = ref[:K][elig].astype(np.float64) / t[:K][elig].astype(np.float64)
                out[i, 0] = np.float32((s * w).sum() / w.sum())
    return out


def ring_tails(rings, ws_K, ws_S, q_ppm, rows_active=0):
    """[local_ranks, K+S] tail rows of NumPy rings (``OracleRings``), packed by gid."""
    KS = ws_K + ws_S
    out = np.full((rings.local_ranks, KS), -1.0, dtype=np.float32)
    counts = np.minimum(rings.total, rings.ring_cap)
    active = rows_active or rings.rows_per_rank
    for lr in range(rings.local_ranks):
        for row in range(active):
            r = lr * rings.rows_per_rank + row
            g = int(rings.gid[r])
            if 0 <= g < KS and counts[r] > 0:
                out[lr, g] = row_quantile(rings.samples[r : r + 1], counts[r : r + 1], q_ppm)[0]
    return out


class _OracleTails:
    def __init__(self, tails, scores, first_rank, n_ranks, q_ppm):
        self._rec = (tails, scores)
        self.first_rank, self.n_ranks, self.q_ppm = first_rank, n_ranks, q_ppm
        self.reads = 0

    def records(self):
        self.reads += 1
        return self._rec


class _TailRingsMixin:
    def tail_local(self, ws, q_ppm, rows_active=0, fused=False):
        self.backend.tail_local_calls += 1
        KS = ws.K + ws.S
        if getattr(ws, "_tail_table", None) is None:
            ws._tail_table = torch.zeros((ws.R, KS), dtype=torch.float32)
            ws._tail_send = ws._tail_table if ws.R == ws.local_ranks else torch.zeros((ws.local_ranks, KS), dtype=torch.float32)
        ws._tail_send.copy_(torch.from_numpy(ring_tails(self, ws.K, ws.S, q_ppm, rows_active)))
        return ws._tail_send, ws._tail_table


class TailOracleRings(_TailRingsMixin, OracleRings):
    pass


class TailOracleRingsFused(_TailRingsMixin, OracleRingsFused):
    pass


class TailOracleBackend(OracleBackend):
    """The CPU checker with tail scores (computed at enqueue time, like its scores)."""

    name = "oracle-test+tails"

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.tail_local_calls = 0
        self.tail_score_calls = 0
        self.handles = []

    def make_rings(self, local_ranks, rows_per_rank, ring_cap):
        cls = TailOracleRingsFused if self.emulate_fused else TailOracleRings
        return cls(self, local_ranks, rows_per_rank, ring_cap)

    def tail_score(self, ws, tails, table, first_rank=0, n_ranks=None, q_ppm=0):
        self.tail_score_calls += 1
        n_ranks = ws.R - first_rank if n_ranks is None else n_ranks
        T = tails.numpy().copy()
        sc = tail_scores_table(T, table.numpy().copy(), ws.K, ws.S, first_rank, n_ranks)
        h = _OracleTails(T[first_rank : first_rank + n_ranks], sc, first_rank, n_ranks, q_ppm)
        self.handles.append(h)
        return h


class _RaisingRings(OracleRings):
    def tail_local(self, *a, **kw):
        self.backend.tail_calls += 1
        raise AssertionError("tail_local() called although tail_quantile is off")


class _RaisingRingsFused(OracleRingsFused):
    tail_local = _RaisingRings.tail_local


class CountingTailBackend(OracleBackend):
    """The plain checker plus ``tail_local`` / ``tail_score`` that only count and raise: with the option off nobody may call them."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.tail_calls = 0

    def make_rings(self, local_ranks, rows_per_rank, ring_cap):
        cls = _RaisingRingsFused if self.emulate_fused else _RaisingRings
        return cls(self, local_ranks, rows_per_rank, ring_cap)

    def tail_score(self, *a, **kw):
        self.tail_calls += 1
        raise AssertionError("tail_score() called although tail_quantile is off")
