"""GPU parity of the timeline scores: ``k_row_timeline`` and ``k_timeline_rank`` against NumPy bit for bit, ``k_timeline_score``
against float64 on planted masks, and one planted window end to end."""
import numpy as np
import pytest
import torch

from nvrx_straggler import _native

pytestmark = pytest.mark.gpu

CAP = _native.MAX_RING_CAP
BUCKETS = (4, 5, 32, 64)
EFFECT = 30000


@pytest.fixture(scope="module")
def be():
    from nvrx_straggler.backend import get_backend

    return get_backend()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _lower_median(v):
    return np.sort(v)[(len(v) - 1) // 2]


def _row_timeline(x, B):
    """The header's step 1 in float64 NumPy: ``x`` in time order -> B ratios, or B times -1."""
    n = len(x)
    if n < 4 * B:
        return np.full(B, -1.0, np.float32)
    edge = [(b * n + B - 1) // B for b in range(B + 1)]  # bucket of i is i * B // n
    with np.errstate(invalid="ignore"):
        m = np.array([x[lo:hi].astype(np.float64).sum() / (hi - lo) for lo, hi in zip(edge, edge[1:])]).astype(np.float32)
    c = _lower_median(m)
    if not np.isfinite(m).all() or c <= 0:
        return np.full(B, -1.0, np.float32)
    return (m.astype(np.float64) / np.float64(c)).astype(np.float32)


@pytest.mark.parametrize("stride", [4096, 4100, CAP])  # the 256-thread variant, the first stride of the 1024-thread one, the cap
def test_row_timeline_is_the_numpy_restatement_bit_for_bit_whatever_the_ring_start(be, stride):
    """Rows are "timings" of 1000 us +- 1 % and one of 600 us +- 1 %: f32 values of two binades, multiples of 2^-14 below
    2^11.  A sum of up to 65 536 of them takes 41 bits, so every f64 bucket sum is exact whatever its order and the comparison
    needs no tolerance.  Also an all-equal row and a row with one infinity (out: all -1)."""
    rng = np.random.default_rng(stride)
    for B in BUCKETS:
        counts = [n for n in (0, 4 * B - 1, 4 * B, 4 * B + 1, 1025, 4095, 4096, 4100, 10001, CAP) if n <= stride]
        counts += [counts[-1]] * 3  # full rows: all equal, one inf, 600 us
        rows = len(counts)
        m = (1000.0 * (1.0 + 0.01 * rng.standard_normal((rows, stride)))).astype(np.float32)
        m[-3] = 1234.5
        m[-2, stride // 3] = np.inf
        m[-1] *= np.float32(0.6)
        exp = np.stack([_row_timeline(m[r, :n], B) for r, n in enumerate(counts)], axis=1)
        assert (exp[:, -3] == 1.0).all() and (exp[:, -2] == -1.0).all() and (exp[:, :2] == -1.0).all() and (exp[:, 2:-2] > 0).all()
        c = torch.tensor(counts, dtype=torch.int32).cuda()
        got = be.row_timeline(torch.from_numpy(m).cuda(), c, B).cpu().numpy()
        assert got.shape == (B, rows) and np.array_equal(_bits(got), _bits(exp)), (B, np.argwhere(_bits(got) != _bits(exp)))
        # the same windows in wrapped rings: slot (start + i) % n holds sample i
        starts = np.array([0 if n == 0 else (7 * r + n // 3) % n for r, n in enumerate(counts)], dtype=np.int32)
        ring = m.copy()
        for r, n in enumerate(counts):
            ring[r, (starts[r] + np.arange(n)) % max(n, 1)] = m[r, :n]
        got = be.row_timeline(torch.from_numpy(ring).cuda(), c, B, torch.from_numpy(starts).cuda()).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(exp)), (B, "wrapped", np.argwhere(_bits(got) != _bits(exp)))


@pytest.mark.parametrize("S", [0, 3])
@pytest.mark.parametrize("K", [0, 1, 2, 65, _native.MAX_ROWS])  # one wave; 256 threads with keys in registers; 1024 re-reading
def test_timeline_rank_is_numpy_sort_and_count_bit_for_bit(be, K, S):
    ranks, B = 3, 5
    rng = np.random.default_rng(K + S)
    planes = (1.0 + 0.05 * rng.standard_normal((ranks, B, K + S))).astype(np.float32)
    planes[rng.random(planes.shape) < 0.2] = -1.0  # holes
    planes[1] = -1.0  # a rank without rows
    planes[0, 0, :K] = np.float32(1.03)  # ties, at the threshold: none is above it
    above = np.float32(1.0 + EFFECT / 1e6)
    exp = np.empty((ranks, 2, 3, B), np.float32)
    for r in range(ranks):
        for f, cols in enumerate((slice(0, K), slice(K, K + S))):
            for b in range(B):
                v = planes[r, b, cols]
                v = v[v >= 0]
                exp[r, f, :, b] = (len(v), _lower_median(v) if len(v) else -1.0, (v > above).sum())
    got = be.timeline_rank(torch.from_numpy(planes).cuda(), K, S, EFFECT).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(exp)), np.argwhere(_bits(got) != _bits(exp))
    assert (exp[1, :, 0] == 0).all() and (exp[0, 0, 2, 0] == 0 or K == 0)


MASKS = {  # B -> the slow buckets planted in rank 1's kernel family, and the run they must give (first, length)
    8: [((), (0, 0)), ((2, 3, 4), (2, 3)), ((0, 1, 4, 5), (4, 2)), ((0, 1, 2, 5), (0, 3)), ((1, 5, 6, 7), (5, 3))],
    64: [(tuple(range(64)), (0, 64)), ((0, 62, 63), (62, 2))],
}


@pytest.mark.parametrize("R", [1, 5, 65])
@pytest.mark.parametrize("B", sorted(MASKS))
def test_timeline_score_on_planted_masks_against_float64(be, R, B):
    """``rel_b`` is one f64 quotient rounded to f32: bit-exact.  ``excess`` is an f64 mean of at most 64 such values rounded to
    f32, the kind of sum behind the GPU score of tests/test_gpu_tail.py: its tolerance, 2e-6.  A job of one rank reads 1.0."""
    min_rows, breadth_ppm = 8, 900000
    rng = np.random.default_rng(R * B)
    me = min(1, R - 1)
    ws = be.workspace(R, 3, 2, R, 0)
    ws.timeline_settle()
    _, _, table, _ = ws.timeline_buffers(B)
    for planted, run in MASKS[B]:
        blocks = np.empty((R, 2, 3, B), np.float32)
        blocks[:, :, 0], blocks[:, :, 2] = 10.0, 9.0  # 9 of 10 rows slower: exactly the breadth asked for
        blocks[:, :, 1] = (1.0 + 0.01 * rng.random((R, 2, B))).astype(np.float32)  # levels within 1 % of each other
        blocks[me, 0, 1, list(planted)] = (1.06 + 0.01 * rng.random(len(planted))).astype(np.float32)
        blocks[me, 1, 1, 2], blocks[me, 1, 2, 2] = 1.06, 8.0  # high, but in 8 of its 10 rows only: not slow
        blocks[-1, 1, 0, 3], blocks[-1, 1, 1, 3] = 7.0, 0.5  # too few rows: not rated, and no reference for the others
        table.copy_(torch.from_numpy(blocks.reshape(R, -1)))
        torch.cuda.synchronize()
        kept, rec = be.timeline_score(ws, table, 0, None, min_rows, EFFECT, breadth_ppm).records()
        assert np.array_equal(_bits(kept), _bits(blocks)) and rec.shape == (R, 2, 4 + B)
        rows, level, slower = blocks[:, :, 0], blocks[:, :, 1], blocks[:, :, 2]
        rated = rows >= min_rows
        ref = np.where(rated, level, np.inf).min(axis=0)
        rel = np.where(rated, (level.astype(np.float64) / ref).astype(np.float32), np.float32(np.nan))
        assert np.array_equal(_bits(rec[:, :, 4:].view(np.float32)), _bits(rel)) and np.isnan(rel[-1, 1, 3])
        with np.errstate(invalid="ignore"):
            slow = rated & (rel.astype(np.float64) >= 1.0 + EFFECT / 1e6) & (slower.astype(np.float64) * 1e6 >= breadth_ppm * rows.astype(np.float64))
        for r in range(R):
            for f in range(2):
                runs = [(n, b) for b in range(B) for n in range(1, B - b + 1) if slow[r, f, b:b + n].all()]
                length, first = max(runs, default=(0, 0))  # the longest, among equal ones the most recent
                assert tuple(rec[r, f, :3]) == (slow[r, f].sum(), first, length), (planted, r, f, rec[r, f, :4])
                if R > 1:  # (the rule above gives what was planted)
                    assert (first, length) == (run if (r, f) == (me, 0) else (0, 0))
                mean = rel[r, f, first:first + length].astype(np.float64).mean() if length else 1.0
                assert abs(float(rec[r, f, 3:4].view(np.float32)[0]) - mean) <= 2e-6
    part = be.timeline_score(ws, table, R - 1, 1, min_rows, EFFECT, breadth_ppm).records()[1]  # one rank out of the table
    assert np.array_equal(part, rec[R - 1:])


def test_a_planted_window_through_folded_job(be):
    from nvrx_straggler.folded import FoldedJob

    data = np.full((4, 8, 512), 1000.0, dtype=np.float32)
    data[:, :, 0:32] *= np.float32(1.1)  # a stretch the whole job shares
    data[2, :, 256:320] *= np.float32(1.05)  # rank 2: every section
    data[1, :4, 256:320] *= np.float32(1.05)  # rank 1: half of its sections -- its lower median stays 1.0
    job = FoldedJob(total_ranks=4, sections=8, ring_cap=512, scores_to_compute=("relative_perf_scores",), timeline_scores=True)
    try:
        for lr, r in enumerate(job.logical_ranks()):
            job.load(lr, data[r])
        rep = job.report()
        t = rep.timeline_scores()
        assert t["buckets"] == 32 and t["params"] == {"min_rows": 8, "min_effect": 0.03, "min_breadth": 0.9, "min_buckets": 2}
        slow = float(np.float32(np.float64(np.float32(1050.0)) / np.float64(np.float32(1000.0))))
        for r in range(4):
            gpu, sec = t["ranks"][r]["gpu"], t["ranks"][r]["sections"]
            assert gpu["rows"] == (0,) * 32 and gpu["slow_buckets"] == 0 and all(np.isnan(gpu["timeline"]))  # (no kernel rows)
            assert sec["rows"] == (8,) * 32
            assert sec["timeline"] == tuple(slow if r == 2 and 16 <= b < 20 else 1.0 for b in range(32)), r
            assert sec["breadth"] == tuple(1.0 if b < 2 or (r == 2 and 16 <= b < 20) else 0.5 if r == 1 and 16 <= b < 20 else 0.0
                                           for b in range(32)), r
            assert (sec["slow_buckets"], sec["began_at"], sec["ended_at"], sec["ended_buckets_ago"]) == (
                (4, 0.5, 0.625, 12) if r == 2 else (0, None, None, None))
            assert sec["excess"] == (slow if r == 2 else 1.0)
        found = rep.identify_timeline_stragglers()
        assert sorted(i.rank for i in found["straggler_section_ranks_relative"]) == [2] and found["straggler_gpus_relative"] == set()
        assert found["runs"] == {"gpus": {}, "sections": {2: (16, 4)}}
        assert rep.identify_timeline_stragglers(min_buckets=5)["runs"] == {"gpus": {}, "sections": {}}
        for name in [n for n in dir(rep) if n.startswith("identify_") and n != "identify_timeline_stragglers"]:
            said = getattr(rep, name)()
            assert not any(v for v in said.values() if not isinstance(v, dict) or any(map(bool, v.values()))), (name, said)
    finally:
        job.close()
