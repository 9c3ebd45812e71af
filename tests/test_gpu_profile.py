"""GPU parity of the tail profile: ``k_row_profile`` against ``numpy.sort`` and against ``k_row_quantile``, bit for bit;
``k_profile_score`` against the float64 restatement of the tail score rule, plane by plane; one planted report end to end."""
import numpy as np
import pytest
import torch

from nvrx_straggler import _native
from tail_oracle_backend import tail_scores_table
from test_gpu_score import _random_table

pytestmark = pytest.mark.gpu

CAP = _native.PROFILE_LDS_SAMPLES
FAR = (500000, 600000, 750000, 900000, 990000, 999000, 999999)
Q_SETS = ((950000,), (500000, 999999), FAR, tuple(range(999990, 999997)))  # Q = 1, 2, 7 far apart, 7 that share one sample
# 4096: the 256-thread variant; 4100: the first stride of the 1024-thread one; 16384: rows on both sides of the LDS cap
COUNTS = {4096: (0, 1, 2, 3, 5, 1023, 1024, 1025, 4095, 4096), 4100: (0, 1, 2, 3, 5, 1023, 1024, 1025, 4099, 4100),
          16384: (0, 5, 1025, CAP - 1, CAP, CAP + 4, 10001, 16384)}


@pytest.fixture(scope="module")
def be():
    from nvrx_straggler.backend import get_backend

    return get_backend()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _rows(pattern, rng, rows, stride):
    if pattern == "equal":  # one group in every pass
        return np.full((rows, stride), 1234.5, dtype=np.float32)
    if pattern == "one_ulp":  # the targets separate only in the last pass
        lo = np.float32(1000.0)
        return np.where(rng.random((rows, stride)) < 0.5, lo, np.nextafter(lo, np.float32(2000.0))).astype(np.float32)
    if pattern == "binades":  # ... in the first: both signs, forty binades, both infinities
        m = (rng.choice([-1.0, 1.0], (rows, stride)) * 10.0 ** rng.uniform(-20.0, 20.0, (rows, stride))).astype(np.float32)
        m[:, 0::97], m[:, 1::89] = np.inf, -np.inf
        return m
    return (1000.0 * (1.0 + 0.01 * rng.standard_normal((rows, stride)))).astype(np.float32)  # "timings": 1000 us +- 1 %


@pytest.mark.parametrize("pattern", ["equal", "one_ulp", "binades", "timings"])
@pytest.mark.parametrize("stride", sorted(COUNTS))
def test_row_profile_is_the_sorted_row_and_the_tail_kernel_bit_for_bit(be, stride, pattern):
    counts = np.array(COUNTS[stride], dtype=np.int32)
    m = _rows(pattern, np.random.default_rng(stride + len(pattern)), counts.size, stride)
    ordered = [np.sort(m[r, :n]) for r, n in enumerate(counts)]
    s, c = torch.from_numpy(m).cuda(), torch.from_numpy(counts).cuda()
    for q_ppm in Q_SETS:
        got = be.row_profile(s, c, q_ppm).cpu().numpy()
        assert got.shape == (len(q_ppm), counts.size)
        for j, q in enumerate(q_ppm):
            exp = np.array([row[(q * int(n) + 999999) // 1000000 - 1] if n else -1.0 for row, n in zip(ordered, counts)], np.float32)
            assert np.array_equal(_bits(got[j]), _bits(exp)), (q_ppm, j, counts[_bits(got[j]) != _bits(exp)], got[j], exp)
            assert np.array_equal(_bits(got[j]), _bits(be.row_quantile(s, c, q).cpu().numpy())), (q_ppm, j)


@pytest.mark.parametrize("R", [5, 65])  # 65: the two-stage column minimum
def test_profile_score_is_the_tail_score_rule_plane_by_plane(be, R):
    K, S, Q, q_ppm = 3, 2, 3, (900000, 990000, 999000)
    rng = np.random.default_rng(R)
    T = _random_table(rng, R, K, S, 0.0)  # (every weight present: what is missing here is missing from the profile)
    profile = np.sort(rng.lognormal(1.0, 0.5, (R, Q, K + S)), axis=1).astype(np.float32)
    profile[1, :, 0] = -1.0  # rank 1 has no row for kernel 0: that column has no reference
    profile[3, :, K + 1] = -1.0  # ... and rank 3 none for section 1
    ws = be.workspace(R, K, S, R, 0)
    ws.profile_settle()
    ws.send.copy_(torch.from_numpy(T))
    _, table, _, _ = ws.profile_buffers(Q)
    table.copy_(torch.from_numpy(profile.reshape(R, -1)))
    torch.cuda.synchronize()
    kept, got = be.profile_score(ws, table, ws.send, 0, None, q_ppm).records()
    assert np.array_equal(_bits(kept), _bits(profile)) and got.shape == (R, Q, 1 + S)
    for j in range(Q):
        exp = tail_scores_table(profile[:, j], T, K, S)
        assert np.array_equal(np.isnan(got[:, j]), np.isnan(exp)) and np.isnan(exp[:, 2]).all() and np.isfinite(exp[:, 0]).all()
        sec = ~np.isnan(exp[:, 1:])
        assert np.array_equal(_bits(got[:, j, 1:][sec]), _bits(exp[:, 1:][sec]))  # one f64 quotient rounded to f32
        assert np.abs(got[:, j, 0].astype(np.float64) - exp[:, 0].astype(np.float64)).max() <= 2e-6  # (tests/test_gpu_tail.py's)
    _, part = be.profile_score(ws, table, ws.send, 2, 2, q_ppm).records()  # ranks out of the middle
    assert np.array_equal(_bits(part), _bits(got[2:4]))


SLOW_AT = (3, 17, 40, 41, 97, 150, 151, 152, 230, 299, 333, 398)  # 12 of 400 samples: 3 %


def _planted():
    """4 ranks x 2 sections x 400 samples without noise; rank 2 is 1.5 x slower at SLOW_AT."""
    data = np.empty((4, 2, 400), dtype=np.float32)
    data[:, 0], data[:, 1] = 1000.0, 2500.0
    data[2][:, list(SLOW_AT)] *= np.float32(1.5)
    return data


def test_a_planted_window_through_folded_job(be):
    from nvrx_straggler.folded import FoldedJob

    data, qs = _planted(), (0.9, 0.99, 0.999)
    # NumPy first: ranks 359, 395 and 399 of 400 -- the 0.9-quantile is a base sample on every rank, the other two are slow ones
    ranks = [_native.tail_rank(q, 400) for q in _native.profile_q_ppm(qs)]
    assert ranks == [359, 395, 399]
    t = np.sort(data, axis=2)[:, :, ranks]  # [4, 2, 3]
    assert (t[2] == t[0] * np.float32([1.0, 1.5, 1.5])).all() and (t[[1, 3]] == t[0]).all()
    names = ["section_000", "section_001"]
    job = FoldedJob(total_ranks=4, sections=2, ring_cap=400, scores_to_compute=("relative_perf_scores",), tail_profile=qs)
    try:
        for lr, r in enumerate(job.logical_ranks()):
            job.load(lr, data[r])
        rep = job.report()
        p = rep.tail_profile()
        assert p["quantiles"] == qs and p["kernel_profile"] == {} and sorted(p["section_profile"]) == names
        slow = float(np.float32(np.float64(1.0) / np.float64(np.float32(1.5))))
        for s, n in enumerate(names):
            for r in range(4):
                assert p["section_profile"][n][r] == tuple(map(float, t[r, s])), (n, r)
                assert p["section_relative"][n][r] == ((1.0, slow, slow) if r == 2 else (1.0, 1.0, 1.0)), (n, r)
        found = rep.identify_tail_profile_stragglers()
        assert {n: sorted(i.rank for i in v) for n, v in found["straggler_sections_relative"].items()} == {n: [2] for n in names}
        assert found["straggler_gpus_relative"] == set()  # (no kernel rows: the GPU scores are NaN)
        assert found["slow_share"] == {"gpus": {}, "sections": {n: {2: (0.01, 0.1)} for n in names}}
        assert rep.tail_scores() == {} and not any(rep.identify_tail_stragglers().values())
        assert not any(rep.identify_stragglers().values())
    finally:
        job.close()
