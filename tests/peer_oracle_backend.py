"""Peer-group scores for the CPU checker backend, and the NumPy restatement the peer tests compare against -- TEST
INFRASTRUCTURE, lives outside the product.

``peer_group_arrays`` / ``peer_columns`` / ``peer_scores_table`` restate the contract of include/nvrx_straggler.h
(``nvrx_peer_score``) in NumPy and plain Python: the floor is found by ``f2key`` (tail_oracle_backend), the quotients are f64
rounded to f32, the GPU slot is a SEQUENTIAL f64 sum over the kernel ids in ascending order -- nothing is shared with the
kernels' wave layout.  The guards on the array's contents are restated too (a group id outside [0, G): NaN; a member outside
[0, R): skipped; start clamped to [0, R]).  ``PeerOracleBackend`` / its rings are the checker with everything a report can
carry (``SlackOracleBackend``) plus ``peer_score`` / ``report_peer`` built on the restatement, so that the host side of the
feature runs on a box without a GPU.  ``CountingPeerBackend`` has peer methods that only count and raise: with the option off
nobody may call them.  ``stage_medians`` is the issue's sketch: 8 ranks, two pipeline stages, rank 6 slow within its stage.
"""
import numpy as np

from slack_oracle_backend import SlackOracleBackend, SlackOracleRings, SlackOracleRingsFused
from tail_oracle_backend import f2key, key2f

NAN32 = np.float32(np.nan)
NAN_BITS = np.uint32(0x7FC00000)

STAGE_RANKS, STAGE_SLOW_RANK = 8, 6


def stage_medians(noise=0.0, seed=5, sections=1):
    """``[8, sections]`` f64 microseconds: ranks 0-3 run a stage of 1000 us, ranks 4-7 one of 1500 us, rank 6 is 1.4 x slower
    than its stage's peers; ``noise``: relative sigma."""
    rng = np.random.default_rng(seed)
    med = np.repeat(np.array([1000.0] * 4 + [1500.0] * 4)[:, None], sections, axis=1)
    med[STAGE_SLOW_RANK] *= 1.4
    return med * (1.0 + noise * rng.standard_normal(med.shape))


def peer_group_arrays(labels):
    """``(arrays, names)``: ``group[R] | members[R] | start[G+1]`` int32 for one label per rank -- dense ids in order of first
    appearance by ascending rank, members sorted by (group id, rank) -- and the labels by id."""
    names = []
    for lab in labels:
        if lab not in names:
            names.append(lab)
    group = [names.index(lab) for lab in labels]
    members = sorted(range(len(labels)), key=lambda r: (group[r], r))
    start = [0]
    for g in range(len(names)):
        start.append(start[-1] + group.count(g))
    return np.array(group + members + start, dtype=np.int32), names


def _stretch(arrays, R, G, g):
    start = arrays[2 * R : 2 * R + G + 1]
    s0, s1 = (min(max(int(x), 0), R) for x in (start[g], start[g + 1]))
    return [int(m) for m in arrays[R + s0 : R + max(s0, s1)]], max(0, s1 - s0)


def peer_columns(T, K, S, arrays, G, min_ranks):
    """``[G, K+S, 4]`` uint32 column records {f32 floor, u32 present, i32 floor_rank, u32 members} of the f32 table ``T``."""
    T = np.asarray(T, dtype=np.float32)
    R, KS = T.shape[0], K + S
    out = np.zeros((G, KS, 4), dtype=np.uint32)
    for g in range(G):
        members, n_members = _stretch(arrays, R, G, g)
        members = np.array(sorted(m for m in members if 0 <= m < R), dtype=np.int64)  # ascending: argmin finds the lowest rank
        out[g, :, 3] = n_members
        out[g, :, 0], out[g, :, 2] = NAN_BITS, np.uint32(0xFFFFFFFF)
        if members.size == 0 or KS == 0:
            continue
        sub = T[members, :KS]
        with np.errstate(invalid="ignore"):
            here = sub >= 0  # the -1 sentinel and NaN are absent
        present = here.sum(axis=0)
        keys = np.where(here, f2key(sub).reshape(sub.shape).astype(np.int64), np.int64(1) << 32)  # absent: above every key
        first = np.argmin(keys, axis=0)  # the first of equal keys: the lowest rank
        best = keys[first, np.arange(KS)]
        ref = (present >= min_ranks) & (present > 0)
        out[g, :, 1] = present
        out[g, ref, 0] = key2f(best[ref].astype(np.uint32)).view(np.uint32)
        out[g, ref, 2] = members[first[ref]].astype(np.int32).view(np.uint32)
    return out


def peer_scores_table(T, K, S, arrays, G, first_rank=0, n_ranks=None, min_ranks=2):
    """``(cols [G, K+S, 4] uint32, scores [n_ranks, 1 + S] f32)``: slot 1 + s the quotient floor / v of the rank's own group
    (f64, rounded to f32), slot 0 the weighted mean of the quotients over the eligible kernels, summed sequentially in f64."""
    T = np.asarray(T, dtype=np.float32)
    R, KS = T.shape[0], K + S
    n_ranks = R - first_rank if n_ranks is None else n_ranks
    cols = peer_columns(T, K, S, arrays, G, min_ranks)
    floors = cols[:, :, 0].view(np.float32).astype(np.float64)
    referenced = cols[:, :, 1] >= min_ranks
    out = np.full((n_ranks, 1 + S), NAN32, dtype=np.float32)
    for i in range(n_ranks):
        r = first_rank + i
        g = int(arrays[r])
        if not 0 <= g < G:
            continue
        row = T[r]
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            ok = (row[:KS] >= 0) & referenced[g]
            q = floors[g] / row[:KS].astype(np.float64)
            out[i, 1:] = np.where(ok[K:], q[K:], np.nan).astype(np.float32)
            sw = sq = 0.0
            n = 0
            for k in range(K):
                if ok[k]:
                    w = float(row[2 * KS + k])
                    sq += w * float(q[k])
                    sw += w
                    n += 1
            if n:
                out[i, 0] = np.float32(np.float64(sq) / np.float64(sw))
    return cols, out


class _OraclePeer:
    def __init__(self, rec, first_rank, n_ranks):
        self._rec = rec
        self.first_rank, self.n_ranks = first_rank, n_ranks
        self.reads = 0

    def records(self):
        self.reads += 1
        return self._rec


def _peer(backend, ws, table, groups, first_rank, n_ranks, min_ranks):
    backend.peer_calls += 1
    n_ranks = ws.R - first_rank if n_ranks is None else n_ranks
    assert groups.R == ws.R, (groups.R, ws.R)
    backend.peer_args.append((ws.R, groups.G, first_rank, n_ranks, min_ranks))
    h = _OraclePeer(peer_scores_table(table.numpy().copy(), ws.K, ws.S, groups.host, groups.G, first_rank, n_ranks, min_ranks),
                    first_rank, n_ranks)
    backend.peer_handles.append(h)
    return h


class PeerOracleRings(SlackOracleRings):
    pass


class PeerOracleRingsFused(SlackOracleRingsFused):
    def report_peer(self, ws, groups, first_rank=0, n_ranks=None, min_ranks=2):
        return _peer(self.backend, ws, self._last[0], groups, first_rank, n_ranks, min_ranks)


class PeerOracleBackend(SlackOracleBackend):
    """The CPU checker with everything a report can carry, peer-group scores included (computed at enqueue time)."""

    name = "oracle-test+peer"

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.peer_calls = 0
        self.peer_args, self.peer_handles = [], []

    def make_rings(self, local_ranks, rows_per_rank, ring_cap):
        cls = PeerOracleRingsFused if self.emulate_fused else PeerOracleRings
        return cls(self, local_ranks, rows_per_rank, ring_cap)

    def peer_score(self, ws, table, groups, first_rank=0, n_ranks=None, min_ranks=2):
        return _peer(self, ws, table, groups, first_rank, n_ranks, min_ranks)


class _RaisingPeerRings(SlackOracleRings):
    def report_peer(self, *a, **kw):
        self.backend.peer_calls += 1
        raise AssertionError("report_peer() called although peer_groups is off")


class _RaisingPeerRingsFused(SlackOracleRingsFused):
    report_peer = _RaisingPeerRings.report_peer


class CountingPeerBackend(SlackOracleBackend):
    """The checker with everything else working and peer methods that only count and raise."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.peer_calls = 0

    def make_rings(self, local_ranks, rows_per_rank, ring_cap):
        cls = _RaisingPeerRingsFused if self.emulate_fused else _RaisingPeerRings
        return cls(self, local_ranks, rows_per_rank, ring_cap)

    def peer_score(self, *a, **kw):
        self.peer_calls += 1
        raise AssertionError("peer_score() called although peer_groups is off")
