"""Node scores for the CPU checker backend, and the NumPy restatement the tests compare against -- TEST INFRASTRUCTURE, lives
outside the product.

``node_scores_table`` restates the definitions of include/nvrx_straggler.h (``nvrx_node_score``) in NumPy: block A is
``pace_group_columns`` with ``min_ranks = min_members`` and ``min_peers = 1`` (so the guards on the node array's contents are
that function's), block B a lower median across the referenced pairs of a column, blocks C and D the rank record of
``pace_scores_table`` with another row and another centre (``rank_records``; tests/test_node_host.py holds it against
``pace_scores_table`` itself).  ``NodeOracleBackend`` / its rings are the checker with everything a report can carry
(``PaceGroupOracleBackend``) plus ``node_score`` / ``report_node`` built on them, so that the host side of the feature runs on a
box without a GPU.
"""
import numpy as np

from pace_group_oracle_backend import (PaceGroupOracleBackend, PaceGroupOracleRings, PaceGroupOracleRingsFused,
                                       pace_group_columns)
from robust_oracle_backend import NAN_BITS, lower_median_by_key
from tail_oracle_backend import f2key, key2f


def node_columns(pairs, min_nodes):
    """Block B, ``[K+S, 4]`` uint32 {f32 N_c, u32 nodes, u32 above, u32 below}, of block A ``pairs`` [G, K+S, 4]: a pair is
    referenced where its med is not NaN."""
    G, KS = pairs.shape[:2]
    out = np.zeros((KS, 4), dtype=np.uint32)
    med = np.ascontiguousarray(pairs[:, :, 0]).view(np.float32)
    for c in range(KS):
        v = med[:, c]
        v = v[~np.isnan(v)]
        out[c, 0], out[c, 1] = NAN_BITS, v.size
        if v.size == 0:
            continue
        keys = f2key(v)
        nkey = lower_median_by_key(keys)
        if v.size >= min_nodes:
            out[c, 0] = np.float32(key2f(nkey)).view(np.uint32)
        out[c, 2], out[c, 3] = int((keys > nkey).sum()), int((keys < nkey).sum())
    return out


def rank_records(V, W, ctr, referenced, K, S):
    """``(recs [n, 2, 8] uint32, terms [n, 3] f64)``: ``nvrx_pace_score``'s rank record of every row of ``V`` [n, K+S] (f32
    values, present iff >= 0) against the centres ``ctr`` [K+S] of the columns ``referenced`` [K+S]; ``W`` [n, K] the weights
    of part 0's three sums, or None: the sums stay +0.0.  ``terms`` as ``pace_scores_table`` gives them."""
    V = np.asarray(V, dtype=np.float32)
    n, KS = V.shape[0], K + S
    recs = np.zeros((n, 2, 8), dtype=np.uint32)
    f = recs.view(np.float32)
    terms = np.zeros((n, 3), dtype=np.float64)
    for i in range(n):
        for p, (lo, hi) in enumerate(((0, K), (K, KS))):
            v, c = V[i, lo:hi], ctr[lo:hi]
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
            if p == 0 and W is not None:
                w = W[i].astype(np.float64)
                with np.errstate(invalid="ignore", over="ignore"):
                    ex = w[has_q] * (1.0 - quot[has_q])
                    f[i, p, 5], f[i, p, 6], f[i, p, 7] = w[eligible].sum(), w[slower].sum(), ex.sum()
                    terms[i] = np.abs(w[eligible]).sum(), np.abs(w[slower]).sum(), np.abs(ex).sum()
    return recs, terms


def node_scores_table(T, K, S, groups, G, max_group, min_members=2, min_nodes=3, first_rank=0, n_ranks=None):
    """``(pairs [G, K+S, 4], cols [K+S, 4], nodes [G, 2, 8], ranks [n_ranks, 2, 8], terms [n_ranks, 3] f64)``: blocks A, B, C
    and D of ``nvrx_node_score`` (uint32 bit patterns) and the magnitudes of the terms of D's three sums."""
    T = np.asarray(T, dtype=np.float32)
    R, KS = T.shape[0], K + S
    n_ranks = R - first_rank if n_ranks is None else n_ranks
    pairs = pace_group_columns(T, K, S, groups, G, max_group, min_members, 1)
    cols = node_columns(pairs, min_nodes)
    ctr = cols[:, 0].copy().view(np.float32)
    referenced = ~np.isnan(ctr)
    med = np.ascontiguousarray(pairs[:, :, 0]).view(np.float32)  # NaN, so not present, where the pair is not referenced
    nodes, _ = rank_records(med, None, ctr, referenced, K, S)
    rows = T[first_rank : first_rank + n_ranks]
    ranks, terms = rank_records(rows[:, :KS], rows[:, 2 * KS : 2 * KS + K], ctr, referenced, K, S)
    return pairs, cols, nodes, ranks, terms


class _OracleNode:
    def __init__(self, rec, first_rank, n_ranks):
        self._rec = rec
        self.first_rank, self.n_ranks = first_rank, n_ranks
        self.reads = 0

    def records(self):
        self.reads += 1
        return self._rec


def _node(backend, ws, table, nodes, first_rank, n_ranks, min_members, min_nodes):
    backend.node_calls += 1
    n_ranks = ws.R - first_rank if n_ranks is None else n_ranks
    assert nodes.R == ws.R, (nodes.R, ws.R)
    backend.node_args.append((ws.R, nodes.G, nodes.max_size, min_members, min_nodes, first_rank, n_ranks))
    rec = node_scores_table(table.numpy().copy(), ws.K, ws.S, nodes.host, nodes.G, nodes.max_size, min_members, min_nodes,
                            first_rank, n_ranks)[:4]
    h = _OracleNode(rec, first_rank, n_ranks)
    backend.node_handles.append(h)
    return h


class NodeOracleRings(PaceGroupOracleRings):
    pass


class NodeOracleRingsFused(PaceGroupOracleRingsFused):
    def report_node(self, ws, nodes, first_rank=0, n_ranks=None, min_members=2, min_nodes=3):
        return _node(self.backend, ws, self._last[0], nodes, first_rank, n_ranks, min_members, min_nodes)


class NodeOracleBackend(PaceGroupOracleBackend):
    """The CPU checker with everything a report can carry, node scores included (computed at enqueue time)."""

    name = "oracle-test+node"

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.node_calls = 0
        self.node_args, self.node_handles = [], []

    def make_rings(self, local_ranks, rows_per_rank, ring_cap):
        cls = NodeOracleRingsFused if self.emulate_fused else NodeOracleRings
        return cls(self, local_ranks, rows_per_rank, ring_cap)

    def node_score(self, ws, table, nodes, first_rank=0, n_ranks=None, min_members=2, min_nodes=3):
        return _node(self, ws, table, nodes, first_rank, n_ranks, min_members, min_nodes)


class _RaisingNodeRings(PaceGroupOracleRings):
    def report_node(self, *a, **kw):
        self.backend.node_calls += 1
        raise AssertionError("report_node() called although node_scores is off")


class _RaisingNodeRingsFused(PaceGroupOracleRingsFused):
    report_node = _RaisingNodeRings.report_node


class CountingNodeBackend(PaceGroupOracleBackend):
    """The checker with everything else working -- pace scores, job-wide and per peer group, included -- and node methods
    that only count and raise: with the option off nobody may call them."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.node_calls = 0

    def make_rings(self, local_ranks, rows_per_rank, ring_cap):
        cls = _RaisingNodeRingsFused if self.emulate_fused else _RaisingNodeRings
        return cls(self, local_ranks, rows_per_rank, ring_cap)

    def node_score(self, *a, **kw):
        self.node_calls += 1
        raise AssertionError("node_score() called although node_scores is off")
