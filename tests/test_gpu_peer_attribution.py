"""Peer attribution on the MI355X (``k_peer_attribute``) through the C ABI, against ``_reference`` below: NumPy f64, per group and
column the present minimum and its lowest rank, then n_k, then a stable sort by (-n_k, id).

Tables: medians and weights are small integers times powers of two, so the order is decided by the inputs; ties are exactly
equal inputs.  A member's median is never below its group's floor, so the one NEGATIVE n_k of every case comes from a negative
weight.  Bounds: ids, floor_rank, present and the eligible count exact; score, lost_us and floor bit for bit (the f64 formula
rounded to f32); share / deficit / explained absolute 2e-6 and W relative 1e-6 (tests/test_gpu_attribution.py: f64 sums in
another order); deficit against 1 - the peer step's GPU score 2e-6 * max(1, |.|) (tests/test_gpu_peer.py)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from nvrx_straggler import _native
from nvrx_straggler._native import PEER_ATTR_TILE as T_

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TOL = 2e-6
GROUP = np.array([0, 0, 0, 0, 1, 1, 1, 2], dtype=np.int32)  # rank 7 is alone: unrated under min_ranks = 2
R, S, G, MIN_RANKS = 8, 2, 3, 2


@pytest.fixture(scope="module")
def be():
    from nvrx_straggler.backend import get_backend

    return get_backend()


def _table(K, group=GROUP, seed=5):
    """[R, L] f32.  Every case: kernel 1 missing on rank 3; kernel 2 on one member of group 1 only (not referenced); kernels 3
    and 4 exactly equal on every rank (a tie); a negative weight on kernel 0 of ranks 1 and 5; and, where K has them, heavy
    slow kernels on ranks 0 and 5 at both sides of every tile edge and in the last slot."""
    rng = np.random.default_rng(seed + K)
    KS = K + S
    T = np.full((len(group), _native.table_len(K, S)), -1.0, dtype=np.float32)
    base = rng.integers(8, 64, KS) * 0.25
    T[:, :KS] = base[None, :] * rng.choice([1.0, 1.25, 1.5, 2.0, 3.0], (len(group), KS))
    T[:, KS : 2 * KS] = T[:, :KS]  # (history minima: the relative family does not read them)
    T[:, 2 * KS : 2 * KS + K] = rng.integers(1, 64, (len(group), K)) * 4.0
    for j, k in enumerate(k for k in (T_ - 1, T_, T_ + 2, 2 * T_ - 1, 2 * T_, K - 1) if 5 <= k < K):
        for r in (0, 5):
            T[r, k], T[r, 2 * KS + k] = 8.0 * base[k], float((3 + j + r) << 16)
    T[2, 3], T[2, 2 * KS + 3] = 8.0 * base[3], float(2 << 16)  # (heavy on rank 2: the tie leads its list)
    T[:, 4], T[:, 2 * KS + 4] = T[:, 3], T[:, 2 * KS + 3]
    T[3, 1] = -1.0
    T[[4, 6], 2] = -1.0
    T[[1, 5], 0] = 4.0 * base[0]  # (above their groups' floors: s_k < 1)
    T[1, 2 * KS], T[5, 2 * KS] = -32.0, -8.0
    T[:, 2 * KS + K] = 1.0
    return T


def _reference(T, K, group, n_groups, min_ranks, top_n, first, n):
    KS = K + S
    out = np.zeros((n, 1 + top_n, 8), dtype=np.uint32)
    f, i32 = out.view(np.float32), out.view(np.int32)
    f[:, 1:, 1:5], i32[:, 1:, 0], i32[:, 1:, 5] = np.nan, -1, -1
    for i, r in enumerate(range(first, first + n)):
        members = np.flatnonzero(group == group[r]) if 0 <= group[r] < n_groups else np.empty(0, dtype=np.int64)
        sub = T[members, :K]
        present = sub >= 0
        masked = np.where(present, sub, np.float32(np.inf))
        floor = masked.min(axis=0) if members.size else np.empty(0)
        ks = np.flatnonzero((T[r, :K] >= 0) & (present.sum(axis=0) >= min_ranks)) if members.size else members
        if ks.size == 0:
            f[i, 0, :2] = np.nan
            continue
        w = T[r, 2 * KS + ks].astype(np.float64)
        s = floor[ks].astype(np.float64) / T[r, ks].astype(np.float64)
        nk = w * (1.0 - s) + 0.0  # (-0.0 -> +0.0)
        order = np.lexsort((ks, -nk))[:top_n]
        W = w.sum()
        f[i, 0, 0], f[i, 0, 1], out[i, 0, 2], f[i, 0, 3] = nk.sum() / W, nk[order].sum() / W, ks.size, W
        m = len(order)
        i32[i, 1 : 1 + m, 0], f[i, 1 : 1 + m, 1], f[i, 1 : 1 + m, 2], f[i, 1 : 1 + m, 3] = ks[order], nk[order] / W, s[order], nk[order]
        f[i, 1 : 1 + m, 4] = floor[ks[order]]
        i32[i, 1 : 1 + m, 5] = members[masked.argmin(axis=0)][ks[order]]  # (argmin: the first, so the lowest rank)
        out[i, 1 : 1 + m, 6] = present.sum(axis=0)[ks[order]]
    return out


def _arrays(group, n_groups):
    members = np.argsort(group, kind="stable")
    start = np.searchsorted(group[members], np.arange(n_groups + 1))
    return np.concatenate((group, members, start)).astype(np.int32)


def _run(be, T, K, arrays, n_groups, min_ranks, top_n, first, n, peer_arrays=None):
    """``(records [n, 1 + top_n, 8] uint32, the peer step's GPU scores [R] f32)``: nvrx_peer_score on all ranks (with
    ``peer_arrays`` where the attribution's array is not to be the peer step's), nvrx_peer_attribute behind it."""
    nr = T.shape[0]
    table, d_groups = torch.from_numpy(T).cuda(), torch.from_numpy(arrays).cuda()
    d_peer_groups = d_groups if peer_arrays is None else torch.from_numpy(peer_arrays).cuda()
    peer = torch.zeros(_native.peer_words(n_groups, nr, K, S), dtype=torch.int32, device="cuda")
    out = torch.zeros(_native.peer_attr_words(n, top_n), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    _native.check(be.lib.nvrx_peer_score(table.data_ptr(), nr, K, S, d_peer_groups.data_ptr(), n_groups, 0, nr, min_ranks,
                                         peer.data_ptr(), be._stream_handle))
    _native.check(be.lib.nvrx_peer_attribute(table.data_ptr(), nr, K, S, d_groups.data_ptr(), n_groups, peer.data_ptr(), first, n,
                                             min_ranks, top_n, out.data_ptr(), be._stream_handle))
    be.synchronize()
    scores = peer.cpu().numpy().view(np.float32)[4 * n_groups * (K + S) :].reshape(nr, 1 + S)[:, 0]
    return out.cpu().numpy().view(np.uint32).reshape(n, 1 + top_n, 8), scores


def _compare(got, exp, tag):
    gf, ef = got.view(np.float32), exp.view(np.float32)
    assert np.array_equal(got.view(np.int32)[:, 1:, 0], exp.view(np.int32)[:, 1:, 0]), (tag, "ids", got.view(np.int32)[:, 1:, 0])
    assert np.array_equal(got[:, 0, 2], exp[:, 0, 2]), (tag, "eligible")
    assert np.array_equal(got[:, 1:, 2:7], exp[:, 1:, 2:7]), (tag, "score, lost_us, floor, floor_rank, present")
    assert not got[:, :, 7].any() and not got[:, 0, 4:].any(), (tag, "padding")
    for what, g, e in (("share", gf[:, 1:, 1], ef[:, 1:, 1]), ("deficit", gf[:, 0, 0], ef[:, 0, 0]), ("explained", gf[:, 0, 1], ef[:, 0, 1])):
        assert np.array_equal(np.isnan(g), np.isnan(e)), (tag, what, "NaN")
        err = np.abs(g[~np.isnan(e)].astype(np.float64) - e[~np.isnan(e)])
        assert err.size == 0 or err.max() <= _TOL, (tag, what, err.max())
    assert np.allclose(gf[:, 0, 3], ef[:, 0, 3], rtol=1e-6, atol=0), (tag, "W")


@pytest.mark.parametrize("K,top_n", [(5, 8), (70, 1), (70, 16), (1025, 5), (T_, 16), (T_ + 3, 5), (2 * T_ + 1, 16)])
def test_kernel_matches_the_formula(be, K, top_n):
    T, arrays = _table(K), _arrays(GROUP, G)
    for first, n in ((0, R), (2, 5)):
        got, peer = _run(be, T, K, arrays, G, MIN_RANKS, top_n, first, n)
        _compare(got, _reference(T, K, GROUP, G, MIN_RANKS, top_n, first, n), (K, top_n, first, n))
    f, ids = got.view(np.float32), got.view(np.int32)[:, 1:, 0]  # (the sub-range: ranks 2..6)
    assert np.isnan(_reference(T, K, GROUP, G, MIN_RANKS, top_n, 7, 1).view(np.float32)[0, 0, 0])  # rank 7, alone
    assert 1 not in ids[1] and 2 not in ids[3] and got[1, 0, 2] == K - 1  # rank 3 lacks kernel 1; kernel 2 has no reference for rank 5
    assert ids[0, :2].tolist() == [3, 4][:top_n]  # rank 2's tie: the lower id first
    if top_n >= K:
        assert ids[3, K - 2] == 0 and f[3, K - 1, 3] < 0 and ids[3, K - 1] == -1  # rank 5: the negative n_k last, then -1
    deficit = f[:, 0, 0].astype(np.float64)
    print(K, top_n, "max |deficit - (1 - peer score)|", np.abs(deficit - (1.0 - peer[2:7])).max())
    assert (np.abs(deficit - (1.0 - peer[2:7])) <= _TOL * np.maximum(1.0, np.abs(1.0 - peer[2:7]))).all()


@pytest.mark.parametrize("K,top_n", [(70, 5), (1025, 16)])
def test_one_group_of_all_ranks_is_the_job_wide_attribution(be, K, top_n):
    group = np.zeros(R, dtype=np.int32)
    T = _table(K, group)
    T[3, 1], T[[4, 6], 2] = 5.0, 7.0  # every rank holds every kernel
    got, _ = _run(be, T, K, _arrays(group, 1), 1, 1, top_n, 0, R)
    table = torch.from_numpy(T).cuda()
    scratch = torch.empty(33 * K, dtype=torch.float32, device="cuda")
    out = torch.zeros(_native.attr_words(R, top_n), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    _native.check(be.lib.nvrx_attribute(table.data_ptr(), R, K, S, 0, R, top_n, 0, 1, scratch.data_ptr(), out.data_ptr(), be._stream_handle))
    be.synchronize()
    wide = out.cpu().numpy().view(np.uint32).reshape(R, 2, 1 + top_n, 4)[:, 1]
    assert np.array_equal(got[:, 1:, 0], wide[:, 1:, 0]) and (got.view(np.int32)[:, 1:, 0] >= 0).all()
    assert np.array_equal(got[:, 1:, 2:4], wide[:, 1:, 2:4])  # score and lost_us, bit for bit
    assert np.array_equal(got[:, 0, 2], wide[:, 0, 2])
    gf, wf = got.view(np.float32), wide.view(np.float32)
    assert np.abs(gf[:, 0, :2].astype(np.float64) - wf[:, 0, :2]).max() <= _TOL and np.abs(gf[:, 1:, 1].astype(np.float64) - wf[:, 1:, 1]).max() <= _TOL
    assert np.allclose(gf[:, 0, 3], wf[:, 0, 3], rtol=1e-6, atol=0)


def test_group_ids_out_of_range_unrate_their_rank_alone(be):
    K, top_n = 70, 5
    T, good = _table(K), _arrays(GROUP, G)
    intact, _ = _run(be, T, K, good, G, MIN_RANKS, top_n, 0, R)
    bad = good.copy()
    bad[1], bad[5] = G, -1
    got, _ = _run(be, T, K, bad, G, MIN_RANKS, top_n, 0, R, peer_arrays=good)
    others = [r for r in range(R) if r not in (1, 5)]
    assert np.array_equal(got[others], intact[others])
    f = got.view(np.float32)
    assert np.isnan(f[[1, 5], 0, :2]).all() and not got[[1, 5], 0, 2:].any() and (got.view(np.int32)[[1, 5], 1:, 0] == -1).all()


def _example():
    spec = importlib.util.spec_from_file_location("straggler_example", os.path.join(REPO, "examples", "straggler_example.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    return ex


def test_a_report_names_the_planted_kernels_of_rank_6_on_both_paths():
    ex = _example()
    torch.cuda.set_device(0)
    names, med = ex.peer_explain_medians()
    lost = med[6].astype(np.float64) - med[4:8].min(axis=0)  # n_k / calls: w_k = calls * median
    expected = [names[k] for k in np.lexsort((np.arange(len(names)), -lost))[:3]]
    assert set(expected) <= {names[k] for k in ex.PEER_EXPLAIN_SLOW}
    job = ex.peer_explain_job(kernel_attribution=0, peer_attribution=3)
    try:
        general = job.report()
        assert job.reporter._last_plan_fused is False
        ex.peer_explain_load(job)
        planned = job.report()
        assert job.reporter._last_plan_fused is True
        a, b = general.explain_peer_gpu_scores(), planned.explain_peer_gpu_scores()
    finally:
        job.close()
    assert a == b and sorted(a) == list(range(8))
    assert [k["name"] for k in a[6]["kernels"]] == expected and a[6]["group"] == 1 and a[6]["eligible"] == len(names)
    assert all(k["peers_with_kernel"] == 4 and k["floor_rank"] in (4, 5, 7) and 0.70 < k["score"] < 0.73 for k in a[6]["kernels"])
    assert 0.0 <= a[5]["deficit"] < 0.01 < a[6]["deficit"]
    job = ex.peer_explain_job(kernel_attribution=0, peer_attribution=0)
    try:
        assert job.report().explain_peer_gpu_scores() == {}
    finally:
        job.close()
