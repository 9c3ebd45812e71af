"""Pace scores per peer group for the CPU checker backend, and the NumPy restatement the tests compare against -- TEST
INFRASTRUCTURE, lives outside the product.

``pace_group_columns`` / ``pace_group_scores_table`` restate the definitions of include/nvrx_straggler.h
(``nvrx_pace_group_score``) in NumPy, with the guards on the group array's contents: ``start`` clamped to ``[0, R]``, a stretch
clamped to ``max_group``, members outside ``[0, R)`` skipped, a group id outside ``[0, G)`` left without a column.
``PaceGroupOracleBackend`` / its rings are the checker with everything a report can carry (``PaceOracleBackend``) plus
``pace_group_score`` / ``report_pace_group`` built on them, so that the host side of the feature runs on a box without a GPU.
"""
import numpy as np

from pace_oracle_backend import PaceOracleBackend, PaceOracleRings, PaceOracleRingsFused
from robust_oracle_backend import NAN_BITS, lower_median_by_key
from tail_oracle_backend import f2key, key2f


def group_stretches(groups, R, G, max_group):
    """Per group ``(members that are ranks of the table, size)``: the stretch ``members[s .. e)`` with ``s``, ``e`` the start
    words clamped to ``[0, R]``, ``e >= s`` and ``e - s`` clamped to ``max_group``; ``size`` counts skipped entries too."""
    groups = np.asarray(groups, dtype=np.int64)
    members, start = groups[R : 2 * R], groups[2 * R : 2 * R + G + 1]
    out = []
    for g in range(G):
        s, e = int(np.clip(start[g], 0, R)), int(np.clip(start[g + 1], 0, R))
        size = min(max(e - s, 0), max_group)
        m = members[s : s + size]
        out.append((m[(m >= 0) & (m < R)], size))
    return out


def threshold(min_ranks, min_peers, size):
    """Present members a pair needs to be a reference."""
    return max(min_peers, min(min_ranks, size))


def pace_group_columns(T, K, S, groups, G, max_group, min_ranks, min_peers):
    """``[G, K+S, 4]`` uint32 records {f32 ctr, u32 n, u32 above, u32 below} of the f32 table ``T`` [R, L]."""
    T = np.asarray(T, dtype=np.float32)
    R, KS = T.shape[0], K + S
    out = np.zeros((G, KS, 4), dtype=np.uint32)
    for g, (m, size) in enumerate(group_stretches(groups, R, G, max_group)):
        need = threshold(min_ranks, min_peers, size)
        for c in range(KS):
            v = T[m, c]
            with np.errstate(invalid="ignore"):
                v = v[v >= 0]  # the -1 sentinel and NaN are absent
            n = v.size
            out[g, c, 0], out[g, c, 1] = NAN_BITS, n
            if n == 0:
                continue
            keys = f2key(v)
            ckey = lower_median_by_key(keys)
            if n >= need:
                out[g, c, 0] = np.float32(key2f(ckey)).view(np.uint32)
            out[g, c, 2], out[g, c, 3] = int((keys > ckey).sum()), int((keys < ckey).sum())
    return out


def pace_group_scores_table(T, K, S, groups, G, max_group, first_rank=0, n_ranks=None, min_ranks=4, min_peers=2):
    """``(cols [G, K+S, 4] uint32, recs [n_ranks, 2, 8] uint32, terms [n_ranks, 3] f64)``: ``pace_scores_table``'s rank
    records and ``terms`` with the centre of the rank's own group, over the columns where the rank is present and its group's
    pair is referenced."""
    T = np.asarray(T, dtype=np.float32)
    R, KS = T.shape[0], K + S
    n_ranks = R - first_rank if n_ranks is None else n_ranks
    cols = pace_group_columns(T, K, S, groups, G, max_group, min_ranks, min_peers)
    group = np.asarray(groups[:R], dtype=np.int64)
    need = [threshold(min_ranks, min_peers, size) for _, size in group_stretches(groups, R, G, max_group)]
    recs = np.zeros((n_ranks, 2, 8), dtype=np.uint32)
    f = recs.view(np.float32)
    terms = np.zeros((n_ranks, 3), dtype=np.float64)
    for i in range(n_ranks):
        row = T[first_rank + i]
        g = int(group[first_rank + i])
        in_group = 0 <= g < G
        ctr = cols[g if in_group else 0, :, 0].copy().view(np.float32)
        referenced = (cols[g, :, 1] >= need[g]) if in_group else np.zeros(KS, dtype=bool)
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


class _OraclePaceGroup:
    def __init__(self, rec, first_rank, n_ranks):
        self._rec = rec
        self.first_rank, self.n_ranks = first_rank, n_ranks
        self.reads = 0

    def records(self):
        self.reads += 1
        return self._rec


def _pace_group(backend, ws, table, groups, first_rank, n_ranks, min_ranks, min_peers):
    backend.pace_group_calls += 1
    n_ranks = ws.R - first_rank if n_ranks is None else n_ranks
    assert groups.R == ws.R, (groups.R, ws.R)
    backend.pace_group_args.append((ws.R, groups.G, groups.max_size, first_rank, n_ranks, min_ranks, min_peers))
    rec = pace_group_scores_table(table.numpy().copy(), ws.K, ws.S, groups.host, groups.G, groups.max_size, first_rank, n_ranks,
                                  min_ranks, min_peers)[:2]
    h = _OraclePaceGroup(rec, first_rank, n_ranks)
    backend.pace_group_handles.append(h)
    return h


class PaceGroupOracleRings(PaceOracleRings):
    pass


class PaceGroupOracleRingsFused(PaceOracleRingsFused):
    def report_pace_group(self, ws, groups, first_rank=0, n_ranks=None, min_ranks=4, min_peers=2):
        return _pace_group(self.backend, ws, self._last[0], groups, first_rank, n_ranks, min_ranks, min_peers)


class PaceGroupOracleBackend(PaceOracleBackend):
    """The CPU checker with everything a report can carry, pace scores per peer group included (computed at enqueue time)."""

    name = "oracle-test+pace-group"

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.pace_group_calls = 0
        self.pace_group_args, self.pace_group_handles = [], []

    def make_rings(self, local_ranks, rows_per_rank, ring_cap):
        cls = PaceGroupOracleRingsFused if self.emulate_fused else PaceGroupOracleRings
        return cls(self, local_ranks, rows_per_rank, ring_cap)

    def pace_group_score(self, ws, table, groups, first_rank=0, n_ranks=None, min_ranks=4, min_peers=2):
        return _pace_group(self, ws, table, groups, first_rank, n_ranks, min_ranks, min_peers)


class _RaisingPaceGroupRings(PaceOracleRings):
    def report_pace_group(self, *a, **kw):
        self.backend.pace_group_calls += 1
        raise AssertionError("report_pace_group() called although pace_peer_groups is off")


class _RaisingPaceGroupRingsFused(PaceOracleRingsFused):
    report_pace_group = _RaisingPaceGroupRings.report_pace_group


class CountingPaceGroupBackend(PaceOracleBackend):
    """The checker with everything else working -- peer and job-wide pace scores included -- and grouped pace methods that
    only count and raise: with the option off nobody may call them."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.pace_group_calls = 0

    def make_rings(self, local_ranks, rows_per_rank, ring_cap):
        cls = _RaisingPaceGroupRingsFused if self.emulate_fused else _RaisingPaceGroupRings
        return cls(self, local_ranks, rows_per_rank, ring_cap)

    def pace_group_score(self, *a, **kw):
        self.pace_group_calls += 1
        raise AssertionError("pace_group_score() called although pace_peer_groups is off")
