"""Work groups for the CPU checker backend, and the NumPy restatement the work-group tests compare against -- TEST
INFRASTRUCTURE, lives outside the product.

``work_signature`` / ``work_pair`` / ``work_block`` restate the contract of include/nvrx_straggler.h (``nvrx_work_groups``) in
NumPy and plain Python: one f64 division rounded to f32 per signature, the count rule as one f64 product and one comparison,
both thresholds as Python integers, the components by a flood fill over the alike pairs, the nearest rank by a scan in
ascending rank with a strict comparison of cross-multiplied integers.  Nothing is shared with the kernels' tiling.
``work_block`` gives the whole block, parts A to E, as the entry point lays it out.  ``WorkOracleBackend`` / its rings are the
checker with everything a report can carry (``NodeOracleBackend``) plus ``work_groups`` / ``report_work`` built on the
restatement, so that the host side of the feature runs on a box without a GPU.  ``CountingWorkBackend`` has work methods that
only count and raise: with the option off nobody may call them.
"""
import numpy as np

from node_oracle_backend import NodeOracleBackend, NodeOracleRings, NodeOracleRingsFused

WORK_MAX_RANKS = 4096


def work_layout(R, K, S):
    """Offsets, in 32-bit words, of the parts B, C, D, E of a block and its size: every part starts on a 16-byte boundary."""
    T, KS = -(-R // 64), K + S
    pad4 = lambda n: (n + 3) & ~3  # noqa: E731
    adj = pad4(R * KS)
    part = adj + pad4(2 * R * T)
    rank = part + 4 * R * T
    job = rank + 8 * R
    return {"adj": adj, "part": part, "rank": rank, "job": job, "words": job + 4, "T": T}


def work_signature(T, K, S):
    """``[R, K+S]`` f32: -1 absent, +0.0 present with an unknown count, else the calls per window ``(f32)((f64)w / (f64)med)``."""
    T = np.asarray(T, dtype=np.float32)
    R, KS = T.shape[0], K + S
    sig = np.full((R, KS), -1.0, dtype=np.float32)
    for r in range(R):
        for c in range(KS):
            med = T[r, c]
            if not med >= 0:  # (a NaN is absent)
                continue
            sig[r, c] = 0.0
            if c >= K:
                continue
            w = T[r, 2 * KS + c]
            if med > 0 and np.isfinite(w) and w > 0:
                with np.errstate(over="ignore", under="ignore"):
                    q = np.float32(np.float64(w) / np.float64(med))
                if np.isfinite(q) and q > 0:
                    sig[r, c] = q
    return sig


def work_pair(sa, sb, count_tol):
    """``(unlike, either)`` of two signature rows."""
    pa, pb = sa >= 0, sb >= 0
    either = int(np.count_nonzero(pa | pb))
    unlike = int(np.count_nonzero(pa != pb))
    factor = np.float64(1.0) + np.float64(np.float32(count_tol))
    for c in np.flatnonzero(pa & pb & (sa > 0) & (sb > 0)):
        hi, lo = np.float64(max(sa[c], sb[c])), np.float64(min(sa[c], sb[c]))
        if hi > factor * lo:
            unlike += 1
    return unlike, either


def work_pairs(sig, count_tol):
    """``(unlike [R, R], either [R, R])`` int64: ``work_pair`` for every pair, one rank against all others at a time; the
    diagonal is not a pair and holds zeros."""
    R = sig.shape[0]
    unlike, either = np.zeros((R, R), dtype=np.int64), np.zeros((R, R), dtype=np.int64)
    factor = np.float64(1.0) + np.float64(np.float32(count_tol))
    present, counted = sig >= 0, sig > 0
    wide = sig.astype(np.float64)
    for a in range(R):
        hi, lo = np.maximum(wide[a], wide), np.minimum(wide[a], wide)
        apart = counted[a] & counted & (hi > factor * lo)
        either[a] = np.count_nonzero(present[a] | present, axis=1)
        unlike[a] = np.count_nonzero((present[a] != present) | apart, axis=1)
        unlike[a, a] = either[a, a] = 0
    return unlike, either


def work_block(T, K, S, count_tol=0.25, max_unlike_ppm=100000):
    """The whole block of ``nvrx_work_groups`` for the f32 table ``T``: ``{"sig" [R, K+S] f32, "adj" [R, T] uint64, "part"
    [R, T, 4] uint32, "ranks" [R, 8] uint32, "job" [4] uint32, "words" the flat uint32 block, "root" [R] int}``."""
    T = np.asarray(T, dtype=np.float32)
    R, KS = T.shape[0], K + S
    lay = work_layout(R, K, S)
    tiles = lay["T"]
    sig = work_signature(T, K, S)
    unlike, either = work_pairs(sig, count_tol)
    alike = (either >= 1) & (unlike * 1000000 <= int(max_unlike_ppm) * either)  # (int64: at most 131072 * 10^6)
    alike[np.arange(R), np.arange(R)] = True
    adj = np.zeros((R, tiles), dtype=np.uint64)
    for a in range(R):
        for b in np.flatnonzero(alike[a]):
            adj[a, b // 64] |= np.uint64(1) << np.uint64(b % 64)
    # components by a flood fill from each rank not yet reached, in ascending order: the seed is the component's lowest rank
    root = np.full(R, -1, dtype=np.int64)
    for seed in range(R):
        if root[seed] >= 0:
            continue
        root[seed] = seed
        todo = [seed]
        while todo:
            a = todo.pop()
            for b in np.flatnonzero(alike[a]):
                if root[b] < 0:
                    root[b] = seed
                    todo.append(int(b))
    size = np.bincount(root, minlength=R)

    def nearest(a, lo, hi):
        best = (0, 0, -1)
        for b in range(lo, min(hi, R)):
            if b == a or either[a, b] < 1:
                continue
            u, e = int(unlike[a, b]), int(either[a, b])
            if best[2] < 0 or u * best[1] < best[0] * e:  # strictly smaller share: a tie keeps the lower rank
                best = (u, e, b)
        return best

    part = np.zeros((R, tiles, 4), dtype=np.uint32)
    ranks = np.zeros((R, 8), dtype=np.uint32)
    for a in range(R):
        for j in range(tiles):
            u, e, b = nearest(a, 64 * j, 64 * j + 64)
            part[a, j] = (u, e, np.int32(b).astype(np.uint32), 0)
        u, e, b = nearest(a, 0, R)
        with np.errstate(invalid="ignore"):
            present = sig[a] >= 0
        ranks[a] = (np.int32(root[a]).astype(np.uint32), size[root[a]], np.count_nonzero(alike[a]) - 1,
                    np.int32(b).astype(np.uint32), u, e, np.count_nonzero(present[:K]), np.count_nonzero(present[K:]))
    roots = np.flatnonzero(root == np.arange(R))
    job = np.array([roots.size, np.count_nonzero(size[roots] == 1), size.max(),
                    np.count_nonzero((ranks[:, 6] | ranks[:, 7]) != 0)], dtype=np.uint32)
    words = np.zeros(lay["words"], dtype=np.uint32)
    words[: R * KS] = sig.reshape(-1).view(np.uint32)
    words[lay["adj"] : lay["adj"] + 2 * R * tiles] = adj.reshape(-1).view(np.uint32)
    words[lay["part"] : lay["rank"]] = part.reshape(-1)
    words[lay["rank"] : lay["job"]] = ranks.reshape(-1)
    words[lay["job"] :] = job
    return {"sig": sig, "adj": adj, "part": part, "ranks": ranks, "job": job, "words": words, "root": root,
            "unlike": unlike, "either": either}


def groups_of(root):
    """``{root: [ranks]}`` of a root array."""
    out = {}
    for r, g in enumerate(np.asarray(root).tolist()):
        out.setdefault(int(g), []).append(r)
    return out


class _OracleWork:
    def __init__(self, rec, count_tol, max_unlike_ppm):
        self._rec = rec
        self.count_tol, self.max_unlike_ppm = count_tol, max_unlike_ppm
        self.reads = 0

    def records(self):
        self.reads += 1
        return self._rec


def _work(backend, ws, table, count_tol, max_unlike_ppm):
    backend.work_calls += 1
    backend.work_args.append((ws.R, ws.K, ws.S, float(count_tol), int(max_unlike_ppm)))
    blk = work_block(table.numpy().copy(), ws.K, ws.S, count_tol, max_unlike_ppm)
    h = _OracleWork((blk["ranks"].copy(), blk["job"].copy()), float(count_tol), int(max_unlike_ppm))
    backend.work_handles.append(h)
    return h


class WorkOracleRings(NodeOracleRings):
    pass


class WorkOracleRingsFused(NodeOracleRingsFused):
    def report_work(self, ws, count_tol=0.25, max_unlike_ppm=100000):
        return _work(self.backend, ws, self._last[0], count_tol, max_unlike_ppm)


class WorkOracleBackend(NodeOracleBackend):
    """The CPU checker with everything a report can carry, work groups included (computed at enqueue time)."""

    name = "oracle-test+work"

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.work_calls = 0
        self.work_args, self.work_handles = [], []

    def make_rings(self, local_ranks, rows_per_rank, ring_cap):
        cls = WorkOracleRingsFused if self.emulate_fused else WorkOracleRings
        return cls(self, local_ranks, rows_per_rank, ring_cap)

    def work_groups(self, ws, table, count_tol=0.25, max_unlike_ppm=100000):
        return _work(self, ws, table, count_tol, max_unlike_ppm)


class _RaisingWorkRings(NodeOracleRings):
    def report_work(self, *a, **kw):
        self.backend.work_calls += 1
        raise AssertionError("report_work() called although work_groups is off")


class _RaisingWorkRingsFused(NodeOracleRingsFused):
    report_work = _RaisingWorkRings.report_work


class CountingWorkBackend(NodeOracleBackend):
    """The checker with everything else working and work methods that only count and raise: with the option off nobody may
    call them."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.work_calls = 0

    def make_rings(self, local_ranks, rows_per_rank, ring_cap):
        cls = _RaisingWorkRingsFused if self.emulate_fused else _RaisingWorkRings
        return cls(self, local_ranks, rows_per_rank, ring_cap)

    def work_groups(self, *a, **kw):
        self.work_calls += 1
        raise AssertionError("work_groups() called although work_groups is off")
