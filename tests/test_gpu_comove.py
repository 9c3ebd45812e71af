"""GPU parity of the co-movement groups: ``k_comove_pairs`` (MFMA), the components and the rank records against float64 on
planted unit vectors, ``k_comove_center`` / ``k_comove_unit`` against NumPy, and one planted window end to end."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIMILARITY = 800000
# a seed for which the float64 reference alone keeps every similarity 1e-5 away from the threshold and every row's best
# partner 1e-5 ahead of its second best, at every shape below (asserted in the test, on the reference)
SEED = 0


@pytest.fixture(scope="module")
def be():
    from nvrx_straggler.backend import get_backend

    return get_backend()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def planted_units(R, B, seed):
    """X [R, 64] f32: rows 0..2 a chain A~B~C with A!~C (at 0, 35 and 68 degrees), 3 a zero row, 4 and 5 identical, 7 the
    opposite of 6, ranks 62..66 in one group across the tile edge, the rest two noisy groups and zero rows; normalised in
    f64, rounded to f32, zero from bucket B on."""
    rng = np.random.default_rng(seed)
    p = np.linalg.qr(rng.standard_normal((B, B)))[0].T  # orthonormal prototypes

    def turn(deg):
        return np.cos(np.radians(deg)) * p[2] + np.sin(np.radians(deg)) * p[3]

    x = np.zeros((R, 64))
    for r in range(R):
        if r < 3:
            v = turn((0.0, 35.0, 68.0)[r])
        elif r in (4, 5):
            v = turn(-50.0)
        elif r == 7:
            v = -x[6, :B]
        elif r == 3 or (r % 4 == 3 and not 62 <= r <= 66):
            continue
        else:
            v = p[1 if r == 6 or 62 <= r <= 66 or r % 4 == 1 else 0] + 0.3 / np.sqrt(B) * rng.standard_normal(B)
        x[r, :B] = v / np.sqrt((v * v).sum())
    return x.astype(np.float32)


def pair_reference(x, thr):
    """Steps 4 and 5 of the header in float64 on the f32 values of ``x``."""
    R = len(x)
    s = x.astype(np.float64) @ x.astype(np.float64).T
    active = (x != 0).any(axis=1)
    cand = active[:, None] & active[None, :] & ~np.eye(R, dtype=bool)
    edge = cand & (s >= thr)
    label = np.arange(R)
    while True:
        new = np.minimum(label, np.where(edge, label[None, :], R).min(axis=1))
        new = new[new]
        if (new == label).all():
            break
        label = new
    ranked = np.where(cand, s, -np.inf)
    best = np.where(cand.any(axis=1), ranked.argmax(axis=1), -1)
    return s, cand, edge, label, best, np.sort(ranked, axis=1)


@pytest.mark.parametrize("B", [4, 33, 64])
@pytest.mark.parametrize("R", [1, 2, 3, 63, 64, 65, 130])
def test_pairs_groups_and_records_are_the_float64_reference(be, R, B):
    """Tolerance on the best similarity: 65 * 2^-24 < 4e-6 -- gamma_65 * sum |x_i y_i| for at most 64 f32 multiply-adds in any
    order, and sum |x_i y_i| <= 1 for unit vectors.  Derived, not measured.  Everything else is exact, on the condition the
    reference itself meets: no similarity within 1e-5 of the threshold, every best partner 1e-5 ahead of the second best."""
    x = planted_units(R, B, SEED)
    thr = float(np.float32(SIMILARITY / 1e6))
    s, cand, edge, label, best, ranked = pair_reference(x, thr)
    assert not (cand & (np.abs(s - thr) <= 1e-5)).any()
    assert all(ranked[i, -1] - ranked[i, -2] > 1e-5 for i in range(R) if cand[i].sum() >= 2)
    if R >= 8:  # (the plant is what it says)
        assert edge[0, 1] and edge[1, 2] and not edge[0, 2] and not cand[3].any() and abs(s[4, 5] - 1) < 1e-6 and abs(s[6, 7] + 1) < 1e-6
    if R >= 67:
        assert edge[62:67, 62:67].sum() == 20
    rec, adj, part = be.comove_pairs(torch.from_numpy(x).to(be.device), SIMILARITY)
    T = -(-R // 64)
    bits = (adj[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
    assert np.array_equal(bits.reshape(R, 64 * T)[:, :R].astype(bool), edge) and not bits.reshape(R, 64 * T)[:, R:].any()
    size = np.bincount(label, minlength=R)[label]
    assert np.array_equal(rec[:, 0].view(np.int32), label) and np.array_equal(rec[:, 1], size)
    assert np.array_equal(rec[:, 2], edge.sum(axis=1)) and np.array_equal(rec[:, 3].view(np.int32), best)
    best_s = np.where(best >= 0, s[np.arange(R), best], 0.0)
    assert np.abs(rec[:, 4].view(np.float32).astype(np.float64) - best_s).max() < 4e-6 and not rec[:, 5:].any()
    if R >= 3:
        assert rec[0, 2] + 1 < rec[0, 1] == 3  # the chain reads loose: A has one partner in a group of three
    # s[i][j] and s[j][i] come from different tiles (or quadrants) and are the same bits
    mutual = 0
    for i in range(R):
        for t in range(T):
            j = int(part[i, t, 1].view(np.int32))
            if j >= 0 and int(part[j, i // 64, 1].view(np.int32)) == i:
                assert part[i, t, 0] == part[j, i // 64, 0], (i, j)
                mutual += 1
    assert mutual >= (2 if R >= 2 else 0)


def unit_reference(blocks, min_rows, amplitude_ppm):
    """Steps 1 to 3 of the header in NumPy."""
    rows, level = blocks[:, :, 0], blocks[:, :, 1]  # [R, 2, B]
    R, _, B = rows.shape
    rated = rows >= min_rows
    n = rated.sum(axis=0)
    c = np.zeros((2, B), np.float32)
    for f in range(2):
        for b in range(B):
            if n[f, b]:
                c[f, b] = np.sort(level[rated[:, f, b], f, b])[(n[f, b] - 1) // 2]
    on = rated & ((n >= 3) & (c > 0))[None]
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.where(on, (level.astype(np.float64) / c.astype(np.float64)[None] - 1.0).astype(np.float32), np.float32(0))
    peak = np.abs(d).max(axis=2)
    pb = np.abs(d).argmax(axis=2)
    active = peak >= np.float32(amplitude_ppm / 1e6)
    ss = (d.astype(np.float64) ** 2).sum(axis=2)
    with np.errstate(divide="ignore", invalid="ignore"):
        x = np.where(active[:, :, None], (d.astype(np.float64) / np.sqrt(ss)[:, :, None]).astype(np.float32), np.float32(0))
    return c, n, d, peak, pb, active, np.sign(np.take_along_axis(d, pb[:, :, None], axis=2)[:, :, 0]).astype(np.int32), x


@pytest.mark.parametrize("B", [4, 64])
@pytest.mark.parametrize("R", [2, 3, 5, 65])
def test_center_and_unit_timelines_are_the_numpy_restatement(be, R, B):
    """Family 0: noisy levels with holes (unrated ranks; bucket 1 keeps two rated ranks: unusable), one rank that stays below
    the amplitude.  Family 1: an all-equal job but for rank 0, exactly AT the amplitude 2^-6 in bucket 2 (active), and rank 1,
    one ulp below it (inactive).  c, d, peak, its bucket, the sign and the active flag bit for bit; x within 1 ulp (the f64
    sum of squares depends on its order)."""
    rng = np.random.default_rng(100 * R + B)
    min_rows, amplitude_ppm = 8, 15625  # 2^-6
    blocks = np.zeros((R, 2, 3, B), np.float32)
    blocks[:, :, 0] = 8 + rng.integers(0, 3, (R, 2, B))
    blocks[:, 0, 1] = 1.0 + 0.02 * rng.standard_normal((R, B))
    blocks[-1, 0, 1] = 1.0 + 0.001 * rng.standard_normal(B)  # never reaches the amplitude
    blocks[:, 0, 0][rng.random((R, B)) < 0.15] = 7  # holes
    blocks[:2, 0, 0, 1], blocks[2:, 0, 0, 1] = 8, 0
    blocks[:, 1, 1] = 1.0
    blocks[0, 1, 1, 2] = 1.0 + 2.0 ** -6
    blocks[1, 1, 1, 2] = 1.0 + 2.0 ** -6 - 2.0 ** -23
    c, n, d, peak, pb, active, sign, x = unit_reference(blocks, min_rows, amplitude_ppm)
    if R >= 5:  # (the plant is what it says; below, the planted ranks are the job's centre themselves)
        assert active[0, 1] and not active[1, 1] and active[:, 0].any() and n[0, 1] == 2 and not d[:, 0, 1].any()
    if R == 65:
        assert not active[-1, 0]
    g_c, g_n, rec, g_d, g_x = be.comove_unit(torch.from_numpy(blocks).to(be.device), min_rows, amplitude_ppm)
    rec, g_d, g_x = rec.transpose(1, 0, 2), g_d.transpose(1, 0, 2), g_x.transpose(1, 0, 2)  # rank-major, as the reference
    assert np.array_equal(_bits(g_c[:, :B]), _bits(c)) and np.array_equal(g_n[:, :B], n) and not g_n[:, B:].any()
    assert np.array_equal(_bits(g_d[:, :, :B]), _bits(d)) and not g_d[:, :, B:].any() and not g_x[:, :, B:].any()
    assert np.array_equal(rec[:, :, 5], _bits(peak)) and np.array_equal(rec[:, :, 6] & 0xFF, pb)
    assert np.array_equal((rec[:, :, 6] >> 8).astype(bool), active) and np.array_equal(rec[:, :, 7].view(np.int32), sign)
    assert (np.abs(g_x[:, :, :B].astype(np.float64) - x) <= np.spacing(np.abs(x))).all() and active.any() == bool(g_x.any())


def test_a_planted_window_through_folded_job(be):
    from nvrx_straggler.folded import FoldedJob

    data = np.full((6, 8, 512), 1000.0, dtype=np.float32)
    data[:, :, 0:32] *= np.float32(1.1)  # a stretch the whole job shares
    data[2:4, :, 256:320] *= np.float32(1.02)  # ranks 2 and 3 together, below the timeline's 3 %
    data[5, :, 64:128] *= np.float32(1.02)  # rank 5 alone
    job = FoldedJob(total_ranks=6, sections=8, ring_cap=512, scores_to_compute=("relative_perf_scores",), timeline_scores=True,
                    comovement_groups=True)
    try:
        for lr, r in enumerate(job.logical_ranks()):
            job.load(lr, data[r])
        rep = job.report()
        assert rep.identify_timeline_stragglers()["runs"] == {"gpus": {}, "sections": {}}
        c = rep.comovement_groups()
        assert c["buckets"] == 32 and c["params"]["min_amplitude"] == 0.01 and c["params"]["min_similarity"] == 0.8
        assert c["groups"]["gpu"] == {} and list(c["groups"]["sections"]) == [2]  # (no kernel rows)
        g = c["groups"]["sections"][2]
        assert (g["ranks"], g["size"], g["loose"], g["began_at"], g["ended_at"]) == ([2, 3], 2, False, 0.5, 0.625)
        assert abs(g["excess"] - 0.02) < 1e-6 and c["center"]["sections"][2:] == (1.0,) * 30 and c["center"]["sections"][0] > 1.09
        sec = {r: c["ranks"][r]["sections"] for r in range(6)}
        assert [sec[r]["active"] for r in range(6)] == [False, False, True, True, False, True]
        assert (sec[5]["partners"], sec[5]["root"], sec[5]["size"], sec[5]["peak_bucket"], sec[5]["sign"]) == (0, 5, 1, 4, 1)
        assert (sec[2]["best_partner"], sec[3]["best_partner"], sec[2]["peak_bucket"]) == (3, 2, 16)
        assert abs(sec[2]["best_similarity"] - 1.0) < 4e-6 and sec[0]["peak"] == 0.0  # (the shared stretch is nobody's)
        found = rep.identify_comoving_stragglers()
        assert sorted(i.rank for i in found["straggler_section_ranks_comoving"]) == [2, 3]
        assert found["straggler_gpus_comoving"] == set() and found["groups"] == {"gpus": {}, "sections": {2: [2, 3]}}
        assert rep.identify_comoving_stragglers(min_ranks=3)["groups"] == {"gpus": {}, "sections": {}}
    finally:
        job.close()
