"""Episode scores for the CPU checker backend, and the NumPy restatement the episode tests compare against -- TEST
INFRASTRUCTURE, lives outside the product.

``episode_one`` / ``row_episode`` / ``episode_excess`` / ``episode_scores_table`` restate the definitions of
include/nvrx_straggler.h (``nvrx_row_episode``, ``nvrx_episode_score``) in NumPy: one float64 ``cumsum`` over the samples in time
order, pivoted on the first one, ``H_t = n * C_t - t * T`` as two rounded products and a rounded difference, a running minimum of
``H_a`` that lags ``b`` by ``m``.  ``EpisodeOracleBackend`` / ``EpisodeOracleRings`` are ``PeriodOracleBackend`` /
``PeriodOracleRings`` plus ``episode_local`` / ``episode_score`` built on them, so that the host side of the feature (option
plumbing, collectives, names, lifetime, pickling) runs on a box without a GPU.
"""
import numpy as np
import torch

from onset_oracle_backend import time_order
from oracle_backend import OracleBackend, OracleRings, OracleRingsFused
from period_oracle_backend import PeriodOracleBackend, _PeriodRingsMixin
from onset_oracle_backend import _OnsetRingsMixin
from tail_oracle_backend import _TailRingsMixin, tail_scores_table

NAN32 = np.float32(np.nan)
PLANES = 7  # {e, inside, outside, strength, length, ago, n}
MIN_SAMPLES = 8
REC = [("ago", np.uint32), ("length", np.uint32), ("inside", np.float32), ("outside", np.float32), ("strength", np.float32)]


def min_len(len_ppm, n):
    """m = max(8, ceil(len_ppm * n / 1e6)) in integers."""
    return max(MIN_SAMPLES, (int(len_ppm) * int(n) + 999999) // 1000000)


class Episode:
    """Everything the definition yields for one row in time order: the record ``rec`` = (ago, length, inside, outside,
    strength), ``m``, and -- where the row has candidates and is finite -- ``H`` [n + 1], the curve ``M`` over b in
    [2m, n - m] (``M[b - 2m]`` = the largest E of an interval that ends at b), ``A`` = sum |d_i|, the chosen ``a``, ``b``
    (0, 0: none) and the largest excess ``E``."""

    __slots__ = ("rec", "m", "n", "H", "M", "A", "a", "b", "E", "C", "T", "sst")

    def e_at(self, a, b):
        """The definition's E of the interval [a, b)."""
        return (self.H[b] - self.H[a]) / np.float64(self.n)

    def admissible(self, a, b):
        return a >= self.m and b <= self.n - self.m and b - a >= self.m


def episode_one(x, len_ppm):
    """The ``Episode`` of one row given in time order (n >= 1)."""
    x = np.asarray(x, dtype=np.float32)
    n = x.size
    ep = Episode()
    ep.n, ep.m = n, min_len(len_ppm, n)
    ep.H = ep.M = ep.C = None
    ep.a = ep.b = 0
    ep.E = 0.0
    m = ep.m
    x0 = np.float64(x[0])
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        d = x.astype(np.float64) - x0
        T = d.sum()
        sst = ((d - T / n) ** 2).sum()
        ep.T, ep.sst = T, sst
        ep.A = float(np.abs(d).sum())
        if not (np.isfinite(T) and np.isfinite(sst)):
            ep.rec = (0, 0, NAN32, NAN32, NAN32)
            return ep
        mean = np.float32(x0 + T / n)
        if n < 3 * m:
            ep.rec = (0, 0, mean, mean, np.float32(0.0))
            return ep
        C = np.concatenate([[0.0], np.cumsum(d)])
        t = np.arange(n + 1, dtype=np.float64)
        H = np.float64(n) * C - t * T  # (NumPy fuses nothing: two products, one difference)
        ep.H, ep.C = H, C
        low = np.minimum.accumulate(H[m : n - 2 * m + 1])  # low[k] = min H_a over a in [m, m + k]
        M = (H[2 * m : n - m + 1] - low) / np.float64(n)    # b = 2m + k pairs with a <= b - m = m + k
        ep.M = M
        k = int(np.argmax(M))  # (the first of equals: the lowest b)
        if not M[k] > 0.0:
            ep.rec = (0, 0, mean, mean, np.float32(0.0))
            return ep
        if sst == 0.0:
            ep.rec = (0, 0, np.float32(x[0]), np.float32(x[0]), np.float32(0.0))
            return ep
        b = 2 * m + k
        a = m + int(np.argmin(H[m : b - m + 1]))  # (the first of equals: the lowest a)
        E = M[k]
        L = b - a
        s_in = C[b] - C[a]
        inside = np.float32(x0 + s_in / L)
        outside = np.float32(x0 + (T - s_in) / (n - L))
        strength = E * E * n / (np.float64(L) * np.float64(n - L)) / sst
        ep.a, ep.b, ep.E = a, b, float(E)
        ep.rec = (n - b, L, inside, outside, np.float32(strength))
        ep.sst = sst
    return ep


def strength64(ep):
    """The f64 strength of an ``Episode`` that found an interval."""
    L = ep.b - ep.a
    return ep.E * ep.E * ep.n / (np.float64(L) * np.float64(ep.n - L)) / ep.sst


def row_episode(samples, counts, len_ppm, starts=None):
    """``[rows]`` structured records ``{ago, length u32, inside, outside, strength f32}`` of every row (absent: {0, 0, -1, -1,
    -1}) and per row its ``Episode`` (None for an absent row)."""
    samples = np.asarray(samples, dtype=np.float32)
    rows, stride = samples.shape
    out = np.zeros(rows, dtype=REC)
    eps = [None] * rows
    for r, c in enumerate(np.asarray(counts).tolist()):
        n = min(int(c), stride)
        if n == 0:
            out[r] = (0, 0, -1.0, -1.0, -1.0)
            continue
        eps[r] = episode_one(time_order(samples[r], n, 0 if starts is None else starts[r]), len_ppm)
        out[r] = eps[r].rec
    return out, eps


def unpack_records(raw):
    """[rows, 4] int32 records of ``nvrx_row_episode`` -> the structured records of ``row_episode``."""
    raw = np.ascontiguousarray(np.asarray(raw, dtype=np.int32))
    out = np.zeros(raw.shape[0], dtype=REC)
    w = raw[:, 0].view(np.uint32)
    out["ago"], out["length"] = w & 0xFFFF, w >> 16
    out["inside"], out["outside"], out["strength"] = (raw[:, i].copy().view(np.float32) for i in (1, 2, 3))
    return out


def episode_excess(length, inside, outside, strength, min_strength):
    """The effective excess of a record: f32 of the f64 quotient inside / outside where the episode is a convincing
    slow-down."""
    inside, outside, strength = np.float32(inside), np.float32(outside), np.float32(strength)
    with np.errstate(invalid="ignore"):
        if length > 0 and strength >= np.float32(min_strength) and inside > outside and outside > 0:
            return np.float32(np.float64(inside) / np.float64(outside))
    return np.float32(1.0)


def episode_scores_table(episodes, table, K, S, first_rank=0, n_ranks=None):
    """``[n_ranks, 1 + S]`` f32 {GPU episode score, section episode scores} from the episode table ``episodes`` [R, 7, K+S]
    (plane 0: the effective excesses) and the weights in the exchange table ``table`` [R, L]: the tail scores' arithmetic on
    plane 0."""
    episodes = np.asarray(episodes, dtype=np.float32)
    return tail_scores_table(np.ascontiguousarray(episodes[:, 0, :]), table, K, S, first_rank, n_ranks)


def ring_episodes(rings, ws_K, ws_S, len_ppm, min_strength, rows_active=0):
    """[local_ranks, 7, K+S] episode planes of NumPy rings (``OracleRings``), packed by gid."""
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
                ago, length, inside, outside, strength = episode_one(time_order(rings.samples[r], n, start), len_ppm).rec
                out[lr, :, g] = (episode_excess(length, inside, outside, strength, min_strength), inside, outside, strength,
                                 length, ago, n)
    return out


class _OracleEpisodes:
    def __init__(self, episodes, scores, first_rank, n_ranks):
        self._rec = (episodes, scores)
        self.first_rank, self.n_ranks = first_rank, n_ranks
        self.reads = 0

    def records(self):
        self.reads += 1
        return self._rec


class _EpisodeRingsMixin:
    def episode_local(self, ws, len_ppm, min_strength, rows_active=0, fused=False):
        assert self.onset_enabled, "episode_local() before onset_enable(): no ring-start snapshot"
        self.backend.episode_local_calls += 1
        KS = ws.K + ws.S
        if getattr(ws, "_episode_table", None) is None:
            ws._episode_table = torch.zeros((ws.R, PLANES * KS), dtype=torch.float32)
            ws._episode_send = ws._episode_table if ws.R == ws.local_ranks else torch.zeros((ws.local_ranks, PLANES * KS), dtype=torch.float32)
        planes = ring_episodes(self, ws.K, ws.S, len_ppm, min_strength, rows_active)
        ws._episode_send.copy_(torch.from_numpy(planes.reshape(self.local_ranks, PLANES * KS)))
        return ws._episode_send, ws._episode_table


class EpisodeOracleRings(_EpisodeRingsMixin, _PeriodRingsMixin, _OnsetRingsMixin, _TailRingsMixin, OracleRings):
    pass


class EpisodeOracleRingsFused(_EpisodeRingsMixin, _PeriodRingsMixin, _OnsetRingsMixin, _TailRingsMixin, OracleRingsFused):
    pass


class EpisodeOracleBackend(PeriodOracleBackend):
    """The CPU checker with episode scores (computed at enqueue time, like its scores) -- and tail, onset and period scores,
    for the reports that carry several."""

    name = "oracle-test+episodes"

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.episode_local_calls = 0
        self.episode_score_calls = 0
        self.episode_handles = []

    def make_rings(self, local_ranks, rows_per_rank, ring_cap):
        cls = EpisodeOracleRingsFused if self.emulate_fused else EpisodeOracleRings
        return cls(self, local_ranks, rows_per_rank, ring_cap)

    def episode_score(self, ws, episodes, table, first_rank=0, n_ranks=None):
        self.episode_score_calls += 1
        n_ranks = ws.R - first_rank if n_ranks is None else n_ranks
        O = episodes.numpy().copy().reshape(ws.R, PLANES, ws.K + ws.S)
        sc = episode_scores_table(O, table.numpy().copy(), ws.K, ws.S, first_rank, n_ranks)
        h = _OracleEpisodes(O[first_rank : first_rank + n_ranks], sc, first_rank, n_ranks)
        self.episode_handles.append(h)
        return h


class _SpyRings(OracleRings):
    def _spied(self, *a, **kw):
        self.backend.episode_calls += 1
        raise AssertionError("an episode method of the rings was called although episode_detection is off")

    onset_enable = episode_local = _spied


class _SpyRingsFused(OracleRingsFused):
    onset_enable = episode_local = _SpyRings._spied


class SpyEpisodeBackend(OracleBackend):
    """The plain checker plus episode methods that only count and raise: with the option off nobody may call them (the
    ring-start snapshot included)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.episode_calls = 0

    def make_rings(self, local_ranks, rows_per_rank, ring_cap):
        cls = _SpyRingsFused if self.emulate_fused else _SpyRings
        return cls(self, local_ranks, rows_per_rank, ring_cap)

    def episode_score(self, *a, **kw):
        self.episode_calls += 1
        raise AssertionError("episode_score() called although episode_detection is off")
