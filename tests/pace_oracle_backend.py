"""Pace scores for the CPU checker backend, and the NumPy restatement the pace tests compare against -- TEST INFRASTRUCTURE,
lives outside the product.

``pace_columns`` / ``pace_scores_table`` restate the definitions of include/nvrx_straggler.h (``nvrx_pace_score``) in NumPy;
``PaceOracleBackend`` / its rings are the checker with everything a report can carry (``PeerOracleBackend``) plus
``pace_score`` / ``report_pace`` built on them, so that the host side of the feature (option plumbing, collectives, names,
lifetime, pickling) runs on a box without a GPU.
"""
import numpy as np

from peer_oracle_backend import PeerOracleBackend, PeerOracleRings, PeerOracleRingsFused
from robust_oracle_backend import NAN_BITS, lower_median_by_key
from slack_oracle_backend import SlackOracleBackend, SlackOracleRings, SlackOracleRingsFused
from tail_oracle_backend import f2key, key2f


def pace_columns(T, K, S, min_ranks):
    """``[K+S, 4]`` uint32 column records {f32 ctr, u32 n, u32 above, u32 below} of the f32 table ``T`` [R, L]."""
    T = np.asarray(T, dtype=np.float32)
    KS = K + S
    out = np.zeros((KS, 4), dtype=np.uint32)
    for c in range(KS):
        v = T[:, c]
        with np.errstate(invalid="ignore"):
            v = v[v >= 0]  # the -1 sentinel and NaN are absent
        n = v.size
        out[c, 0], out[c, 1] = NAN_BITS, n
        if n == 0:
            continue
        keys = f2key(v)
        ckey = lower_median_by_key(keys)
        if n >= min_ranks:
            out[c, 0] = np.float32(key2f(ckey)).view(np.uint32)
        out[c, 2], out[c, 3] = int((keys > ckey).sum()), int((keys < ckey).sum())
    return out


def pace_scores_table(T, K, S, first_rank=0, n_ranks=None, min_ranks=4):
    """``(cols [K+S, 4] uint32, recs [n_ranks, 2, 8] uint32, terms [n_ranks, 3] f64)``: per reported rank and part (0 the
    kernel columns, 1 the section columns) {f32 pace, f32 spread, u32 columns, u32 slower, u32 faster, f32 total_us,
    f32 slower_us, f32 excess_us}; ``terms`` holds the sums of the MAGNITUDES of the terms of part 0's three sums, which the
    tests' tolerance for a sum taken in another order is relative to."""
    T = np.asarray(T, dtype=np.float32)
    R, KS = T.shape[0], K + S
    n_ranks = R - first_rank if n_ranks is None else n_ranks
    cols = pace_columns(T, K, S, min_ranks)
    ctr = cols[:, 0].copy().view(np.float32)
    referenced = (cols[:, 1] >= min_ranks) & (cols[:, 1] > 0)
    recs = np.zeros((n_ranks, 2, 8), dtype=np.uint32)
    f = recs.view(np.float32)
    terms = np.zeros((n_ranks, 3), dtype=np.float64)
    for i in range(n_ranks):
        row = T[first_rank + i]
        for p, (lo, hi) in enumerate(((0, K), (K, KS))):
            v, c = row[lo:hi], ctr[lo:hi]
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                eligible = (v >= 0) & referenced[lo:hi]
                quot = c.astype(np.float64) / v.astype(np.float64)
                q = quot.astype(np.float32)
                has_q = eligible & ~np.isnan(q)
                slower = eligible & (f2key(v) > f2key(c))
                faster = eligible & (f2key(v) < f2key(c))
            recs[i, p, 2], recs[i, p, 3], recs[i, p, 4] = int(eligible.sum()), int(slower.sum()), int(faster.sum())
            recs[i, p, 0] = recs[i, p, 1] = NAN_BITS
            if has_q.any():
                qs = q[has_q]
                pace = np.float32(key2f(lower_median_by_key(f2key(qs))))
                with np.errstate(invalid="ignore", over="ignore"):
                    dev = (qs - pace).astype(np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)  # fabsf; NaN above +inf
                f[i, p, 0] = pace
                recs[i, p, 1] = lower_median_by_key(dev)
            if p == 0:
                w = row[2 * KS : 2 * KS + K].astype(np.float64)
                with np.errstate(invalid="ignore", over="ignore"):
                    ex = w[has_q] * (1.0 - quot[has_q])
                    f[i, p, 5], f[i, p, 6], f[i, p, 7] = w[eligible].sum(), w[slower].sum(), ex.sum()
                    terms[i] = np.abs(w[eligible]).sum(), np.abs(w[slower]).sum(), np.abs(ex).sum()
    return cols, recs, terms


class _OraclePace:
    def __init__(self, rec, first_rank, n_ranks):
        self._rec = rec
        self.first_rank, self.n_ranks = first_rank, n_ranks
        self.reads = 0

    def records(self):
        self.reads += 1
        return self._rec


def _pace(backend, ws, table, first_rank, n_ranks, min_ranks):
    backend.pace_calls += 1
    n_ranks = ws.R - first_rank if n_ranks is None else n_ranks
    backend.pace_args.append((first_rank, n_ranks, min_ranks))
    h = _OraclePace(pace_scores_table(table.numpy().copy(), ws.K, ws.S, first_rank, n_ranks, min_ranks)[:2], first_rank, n_ranks)
    backend.pace_handles.append(h)
    return h


class PaceOracleRings(PeerOracleRings):
    pass


class PaceOracleRingsFused(PeerOracleRingsFused):
    def report_pace(self, ws, first_rank=0, n_ranks=None, min_ranks=4):
        return _pace(self.backend, ws, self._last[0], first_rank, n_ranks, min_ranks)


class PaceOracleBackend(PeerOracleBackend):
    """The CPU checker with everything a report can carry, pace scores included (computed at enqueue time)."""

    name = "oracle-test+pace"

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.pace_calls = 0
        self.pace_args, self.pace_handles = [], []

    def make_rings(self, local_ranks, rows_per_rank, ring_cap):
        cls = PaceOracleRingsFused if self.emulate_fused else PaceOracleRings
        return cls(self, local_ranks, rows_per_rank, ring_cap)

    def pace_score(self, ws, table, first_rank=0, n_ranks=None, min_ranks=4):
        return _pace(self, ws, table, first_rank, n_ranks, min_ranks)


class _RaisingPaceRings(SlackOracleRings):
    def report_pace(self, *a, **kw):
        self.backend.pace_calls += 1
        raise AssertionError("report_pace() called although pace_scores is off")


class _RaisingPaceRingsFused(SlackOracleRingsFused):
    report_pace = _RaisingPaceRings.report_pace


class CountingPaceBackend(SlackOracleBackend):
    """The checker with everything else working and pace methods that only count and raise: with the option off nobody may
    call them."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.pace_calls = 0

    def make_rings(self, local_ranks, rows_per_rank, ring_cap):
        cls = _RaisingPaceRingsFused if self.emulate_fused else _RaisingPaceRings
        return cls(self, local_ranks, rows_per_rank, ring_cap)

    def pace_score(self, *a, **kw):
        self.pace_calls += 1
        raise AssertionError("pace_score() called although pace_scores is off")
