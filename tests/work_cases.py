"""Named tables of the work-group tests with their expected groups -- TEST INFRASTRUCTURE.  The smallest shapes at which each
kernel of ``nvrx_work_groups`` can go wrong: one partial tile, a full tile, a second tile holding one rank, three tiles with a
column tail, sections only, both thresholds exactly, edge values, ties, chains and more ranks than the components kernel has
threads.  ``CASES[name]`` is ``{"T": f32 table [R, L], "K", "S", "count_tol", "max_unlike_ppm", "groups": {root: [ranks]}}``
plus, where the case is about more than its groups, ``"alike"`` (pairs a < b that must be alike), ``"not_alike"``, ``"nearest"``
(``{rank: (nearest, unlike, either)}``), ``"loose"`` (ranks whose component is no clique) and ``"sig"`` (the expected signature
plane).  Every expectation was written by hand from the rule; tests/test_work_host.py holds the oracle to them on the CPU.
"""
import numpy as np

NAN, INF = float("nan"), float("inf")


def table(med, w=None):
    """The exchanged table ``[R, L]`` f32 for medians ``med [R, K+S]`` and kernel weights ``w [R, K]`` (-1 in ``med``: no
    statistics; the running minima repeat the medians; every rank has its names)."""
    med = np.asarray(med, dtype=np.float32)
    R, KS = med.shape
    K = 0 if w is None else np.asarray(w).shape[1]
    T = np.zeros((R, 2 * KS + K + 1), dtype=np.float32)
    T[:, :KS] = med
    T[:, KS : 2 * KS] = med
    if K:
        T[:, 2 * KS : 2 * KS + K] = np.asarray(w, dtype=np.float32)
    T[:, -1] = 1.0
    return T


def counted(calls, us=50.0, sections=0, slow=None):
    """A table whose kernel column k ran ``calls[r][k]`` times on rank r (0: the rank does not have it) at ``us`` microseconds a
    call, ``slow[r]`` times longer on rank r, with ``sections`` section ids that every rank has."""
    calls = np.asarray(calls, dtype=np.float64)
    R, K = calls.shape
    pace = np.ones(R) if slow is None else np.asarray(slow, dtype=np.float64)
    med = np.where(calls > 0, us * pace[:, None], -1.0)
    w = np.where(calls > 0, calls * us * pace[:, None], 0.0)
    med = np.concatenate([med, np.full((R, sections), 1000.0) * pace[:, None]], axis=1)
    return table(med, w), K, sections


def by_label(labels):
    """``{root: [ranks]}`` for one label per rank: the root is the lowest rank of a label."""
    out, first = {}, {}
    for r, lab in enumerate(labels):
        out.setdefault(first.setdefault(lab, r), []).append(r)
    return out


def _case(T, K, S, groups, count_tol=0.25, max_unlike_ppm=100000, **more):
    return dict(T=T, K=K, S=S, count_tol=count_tol, max_unlike_ppm=max_unlike_ppm, groups=groups, **more)


def readme_scenario(noise=0.01, seed=11):
    """The two-stage job of README's ``--work`` example: 8 ranks, 120 kernel keys and 4 sections.  100 keys are shared and ran
    1600 times on ranks 0-3 and 2400 times on ranks 4-7; 10 keys only stage 0 has, 10 only stage 1; rank 6 is 1.4 x slower in
    everything; ``noise``: the relative sigma of every duration.  ``(T, K, S)``."""
    rng = np.random.default_rng(seed)
    R, K, S = 8, 120, 4
    stage = np.arange(R) // 4
    calls = np.zeros((R, K))
    calls[:, :100] = np.where(stage[:, None] == 0, 1600.0, 2400.0)
    calls[stage == 0, 100:110] = 200.0
    calls[stage == 1, 110:120] = 200.0
    base = rng.uniform(20.0, 400.0, K)
    slow = np.where(np.arange(R) == 6, 1.4, 1.0)
    med = base * slow[:, None] * (1.0 + noise * rng.standard_normal((R, K)))
    avg = med * (1.0 + noise * rng.standard_normal((R, K)))
    sec = np.where(stage[:, None] == 0, 1000.0, 1500.0) * slow[:, None] * (1.0 + noise * rng.standard_normal((R, S)))
    T = table(np.concatenate([np.where(calls > 0, med, -1.0), sec], axis=1), np.where(calls > 0, calls * avg, 0.0))
    return T, K, S


def _build():
    cases = {}
    # one rank; two ranks with nothing present (alone each)
    T, K, S = counted([[3, 5]], sections=1)
    cases["one_rank"] = _case(T, K, S, {0: [0]}, nearest={0: (-1, 0, 0)})
    cases["two_ranks_nothing_present"] = _case(table(np.full((2, 3), -1.0), np.zeros((2, 2))), 2, 1, {0: [0], 1: [1]},
                                               nearest={0: (-1, 0, 0), 1: (-1, 0, 0)})
    cases["no_columns"] = _case(table(np.zeros((3, 0))), 0, 0, {0: [0], 1: [1], 2: [2]})
    # one partial tile: ranks 0-3 have kernels 0-7, ranks 4-7 kernels 4-11: 8 of 16 columns apart
    calls = np.zeros((8, 12))
    calls[:4, :8] = 10
    calls[4:, 4:] = 10
    T, K, S = counted(calls, sections=4)
    cases["partial_tile_8"] = _case(T, K, S, by_label([0] * 4 + [1] * 4), nearest={0: (1, 0, 12), 4: (5, 0, 12), 7: (4, 0, 12)})
    # a full tile: the call counts of all 5 kernels tell four groups apart (100, 200, 300, 400 calls: every ratio above 1.25)
    calls = np.repeat((100.0 * (1 + np.arange(64) % 4))[:, None], 5, axis=1)
    T, K, S = counted(calls, sections=1)
    cases["full_tile_64"] = _case(T, K, S, by_label(list(np.arange(64) % 4)))
    # a second tile holding one rank, which belongs to the even ranks' group of the first tile
    calls = np.repeat((100.0 * (1 + np.arange(65) % 2))[:, None], 3, axis=1)
    T, K, S = counted(calls)
    cases["second_tile_of_one_65"] = _case(T, K, S, by_label(list(np.arange(65) % 2)), nearest={64: (0, 0, 3), 63: (1, 0, 3)})
    # three tiles and a column tail of 6: the groups differ in the two LAST kernel columns (64, 65) only, 2 of 70 columns,
    # which 1 % does not allow
    calls = np.full((130, 66), 40.0)
    calls[:, 64:] = (40.0 * (1 + np.arange(130) % 3))[:, None]
    T, K, S = counted(calls, sections=4)
    cases["three_tiles_tail_130x70"] = _case(T, K, S, by_label(list(np.arange(130) % 3)), max_unlike_ppm=10000)
    # sections only: ranks 0-2 have sections 0-2, ranks 3-5 sections 2-4 (4 of 5 columns apart)
    med = np.full((6, 5), -1.0)
    med[:3, :3] = 7.0
    med[3:, 2:] = 7.0
    cases["sections_only"] = _case(table(med), 0, 5, by_label([0] * 3 + [1] * 3))
    # the README scenario: rank 6 is slow, not different
    T, K, S = readme_scenario()
    cases["readme_two_stages"] = _case(T, K, S, by_label([0] * 4 + [1] * 4))
    T, K, S = readme_scenario()
    T[:, 100:120] = -1.0  # no exclusive keys: the call counts alone
    cases["readme_counts_only"] = _case(T, K, S, by_label([0] * 4 + [1] * 4))
    # a chain: rank i ran kernels 0 .. 2 i - 1 twice as often, so ranks i and k are 2 |i - k| of 80 columns apart; 5 % allows
    # 2 and 4, not 6: one component of diameter 6 in which nobody sees everybody
    calls = np.full((12, 80), 100.0)
    for i in range(12):
        calls[i, : 2 * i] = 200.0
    T, K, S = counted(calls)
    cases["chain_of_12"] = _case(T, K, S, {0: list(range(12))}, max_unlike_ppm=50000, loose=list(range(12)),
                                 alike=[(0, 1), (0, 2), (5, 7)], not_alike=[(0, 3), (4, 8)],
                                 nearest={0: (1, 2, 80), 5: (4, 2, 80), 11: (10, 2, 80)})
    # the count boundary: med = 1, w = 4 against 5 at 0.25 is alike (5 > 1.25 * 4 is false), against the next float above 5
    # it is not; max_unlike_ppm = 0 turns one unlike column into "not alike"
    up = np.nextafter(np.float32(5.0), np.float32(INF))
    cases["count_boundary"] = _case(table([[1.0], [1.0], [1.0]], [[4.0], [5.0], [up]]), 1, 0, {0: [0, 1, 2]}, max_unlike_ppm=0,
                                    alike=[(0, 1), (1, 2)], not_alike=[(0, 2)], loose=[0, 2],
                                    sig=np.array([[4.0], [5.0], [up]], dtype=np.float32))
    # the share boundary: 1 unlike column of 10 at 100000 ppm is alike, at 99999 ppm it is not
    med = np.full((2, 10), 3.0)
    med[1, 9] = -1.0
    cases["share_boundary_alike"] = _case(table(med), 0, 10, {0: [0, 1]}, max_unlike_ppm=100000, nearest={0: (1, 1, 10)})
    cases["share_boundary_not_alike"] = _case(table(med), 0, 10, {0: [0], 1: [1]}, max_unlike_ppm=99999, nearest={0: (1, 1, 10)})
    # edge values in med and w: what is present, and what has a count
    med = [[0.0, NAN, INF, -INF, -0.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 1e-30, -1.0, 5.0],
           [2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0, NAN]]
    w = [[8.0, 8.0, 8.0, 8.0, 8.0, 0.0, NAN, INF, -INF, -0.0, -3.0, 3e38, 8.0],
         [8.0, 8.0, 8.0, 8.0, 8.0, 8.0, 8.0, 8.0, 8.0, 8.0, 8.0, 8.0, 8.0]]
    sig = np.array([[0.0, -1.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0],
                    [4.0] * 13 + [-1.0]], dtype=np.float32)  # (3e38 / 1e-30 overflows f32: no count; the section: present / absent)
    cases["edge_values"] = _case(table(med, w), 13, 1, {0: [0], 1: [1]}, sig=sig, nearest={0: (1, 4, 14), 1: (0, 4, 14)})
    # ties for nearest go to the lower rank, also where the equal shares are 1/2 and 2/4
    med = np.full((4, 4), -1.0)
    med[0, :2] = 1.0
    med[1, :1] = 1.0
    med[2, :] = 1.0
    med[3, :1] = 1.0
    cases["nearest_ties"] = _case(table(med), 0, 4, {0: [0], 1: [1, 3], 2: [2]}, nearest={0: (1, 1, 2), 1: (3, 0, 1), 2: (0, 2, 4), 3: (1, 0, 1)})
    # two disjoint cliques whose lowest ranks are interleaved
    calls = np.zeros((10, 6))
    calls[0::2, :4] = 10
    calls[1::2, 2:] = 10
    T, K, S = counted(calls)
    cases["interleaved_cliques"] = _case(T, K, S, by_label(list(np.arange(10) % 2)))
    # more ranks than the components kernel has threads: 18 tiles; five groups by the call counts of both kernels
    calls = np.repeat((100.0 * 2.0 ** (np.arange(1100) % 5))[:, None], 2, axis=1)
    T, K, S = counted(calls, sections=1)
    cases["ranks_1100"] = _case(T, K, S, by_label(list(np.arange(1100) % 5)))
    return cases


CASES = _build()
