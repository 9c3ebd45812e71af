"""GPU parity of the kernels of robust scores per peer group and of the grouped robust step of a report against a NumPy restatement
written here.  Bounds (tests/test_gpu_robust.py's): column records and section scores bit for bit; a NaN the arithmetic itself
makes (inf - inf) by NaN-ness; GPU slots within 2e-6 * max(1, |expected|), an f64 weighted mean summed in another order."""
import numpy as np
import pytest
import torch

from test_gpu_robust import SPECIALS, _bits, _compare, _special
from test_gpu_score import _random_table

pytestmark = pytest.mark.gpu

NAN32 = np.float32(np.nan)
PAD, FILL = 64, 0x5A5A5A5A
# (R, K, S, group sizes): SLOT 4 with a group of one; SLOT 2; SLOT 8, G no multiple of 8, two tiles; SLOT 16 and 32 with short,
# unequal groups (segments at base != 0); SLOT 64; 256 and 1024 threads
CASES = [(7, 3, 2, [1, 2, 4]), (10, 1, 1, [2] * 5), (40, 65, 2, [8] * 5), (40, 2, 2, [16, 11, 13]), (70, 2, 2, [32, 20, 18]),
         (49, 2, 66, [16, 33]), (64, 5, 0, [64]), (70, 2, 1, [65, 5]), (1030, 1, 1, [1025, 5])]


@pytest.fixture(scope="module")
def be():
    from nvrx_straggler.backend import get_backend

    return get_backend()


def _expected(T, K, S, arrays, G, max_group, first, n_ranks, min_ranks, min_peers, floor_rel):
    """``(cols [G, K+S, 4] uint32, scores [n_ranks, 2, 1 + S] f32)`` as include/nvrx_straggler.h defines them, guards included."""
    R, KS = T.shape[0], K + S
    group, members, start = arrays[:R], arrays[R : 2 * R], np.clip(arrays[2 * R :].astype(np.int64), 0, R)
    cols = np.zeros((G, KS, 4), dtype=np.uint32)
    cols[:, :, :3] = NAN32.view(np.uint32)
    for g in range(G):
        size = min(max(int(start[g + 1] - start[g]), 0), max_group)
        mem = [m for m in members[start[g] : start[g] + size] if 0 <= m < R]
        need = max(min_peers, min(min_ranks, size))
        for c in range(KS):
            v = T[mem, c] if mem else np.zeros(0, dtype=np.float32)
            with np.errstate(invalid="ignore"):
                v = v[v >= 0]
                cols[g, c, 3] = n = v.size
                if n < need:
                    continue
                u = v.view(np.uint32)
                ctr = v[np.argsort(np.where(u >> 31, ~u, u | np.uint32(0x80000000)), kind="stable")[(n - 1) >> 1]]  # (f2key)
                mad = np.sort((v - ctr).view(np.uint32) & np.uint32(0x7FFFFFFF))[(n - 1) >> 1].view(np.float32)
                scale = np.fmax(np.float32(1.4826) * mad, np.float32(floor_rel) * ctr)  # (fmaxf: a NaN operand loses)
            cols[g, c, :3] = np.array([ctr, mad, scale], dtype=np.float32).view(np.uint32)
    out = np.full((n_ranks, 2, 1 + S), NAN32, dtype=np.float32)
    for i, r in enumerate(range(first, first + n_ranks)):
        if not 0 <= group[r] < G:
            continue
        f = cols[group[r]].view(np.float32)
        ctr, scale, v = f[:, 0].astype(np.float64), f[:, 2].astype(np.float64), T[r, :KS].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            ok = (T[r, :KS] >= 0) & ~np.isnan(f[:, 0])
            ratio, z = ctr / v, (v - ctr) / scale
            out[i, 0, 1:] = np.where(ok[K:], ratio[K:], np.nan).astype(np.float32)
            out[i, 1, 1:] = np.where(ok[K:], z[K:], np.nan).astype(np.float32)
            e = ok[:K]
            if e.any():
                w = T[r, 2 * KS : 2 * KS + K].astype(np.float64)[e]
                out[i, 0, 0], out[i, 1, 0] = (w * ratio[:K][e]).sum() / w.sum(), (w * z[:K][e]).sum() / w.sum()
    return cols, out


def _case(R, K, S, sizes):
    """Groups shuffled against the table's rows; an all-absent and test_gpu_robust's columns in the smallest and largest group."""
    from nvrx_straggler.backend import PeerGroups

    rng = np.random.default_rng(R * 1000 + K + S)
    labels = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
    groups = PeerGroups(labels.tolist())  # (ids by first appearance: the sizes are asked of it, not assumed)
    by_size = sorted(range(groups.G), key=lambda g: len(groups.members(g)))
    KS, tables, todo = K + S, [], [(kind, g) for kind in ("absent",) + SPECIALS for g in {by_size[0], by_size[-1]}]
    while todo:
        T = _random_table(rng, R, K, S)
        take, todo = todo[:KS], todo[KS:]
        cols = np.linspace(0, KS - 1, len(take)).astype(int) if len(take) > 1 else [KS // 2]
        nan_cols = []
        for c, (kind, g) in zip(cols, take):
            mem = groups.members(g)
            sub = T[mem]
            if kind == "absent":  # nobody of the group has the row: n = 0
                sub[:, int(c)] = -1.0
            else:
                _special(sub, rng, int(c), kind, K, S)
            T[mem] = sub
            if kind == "mostly_inf":
                nan_cols.append(g * KS + int(c))
        tables.append((T, nan_cols))
    return groups, tables


def _run(be, T, K, S, groups, first, n, min_ranks, min_peers, floor_rel=0.02):
    """Through ``backend.robust_group_score``, a guard-padded records buffer planted in the slot: nothing outside it is touched."""
    from nvrx_straggler import _native
    from nvrx_straggler.table_families import ROBUST_GROUP

    R = T.shape[0]
    ws = be.workspace(R, K, S, R, 0)
    ws.robust_settle()
    ws.send.copy_(torch.from_numpy(T))
    words = _native.robust_group_words(groups.G, n, K, S)
    ws.table_buffers(ROBUST_GROUP, n, groups.G)  # (the slot exists; its buffer is replaced by one of the same size)
    big = torch.full((PAD + max(words, 64) + PAD,), FILL, dtype=torch.int32, device="cuda")
    ws._table_state["robust"].buf = big[PAD : PAD + max(words, 64)]
    torch.cuda.synchronize()
    rec = be.robust_group_score(ws, ws.send, groups, first, n, min_ranks, min_peers, floor_rel).records()
    host = big.cpu().numpy()
    assert (host[:PAD] == FILL).all() and (host[PAD + words :] == FILL).all(), (R, K, S, first, n, "outside the block")
    return rec


_flat = lambda rec: (rec[0].reshape(-1, 4), rec[1])  # noqa: E731


@pytest.mark.parametrize("R,K,S,sizes", CASES)
def test_robust_group_score_matches_numpy(be, R, K, S, sizes):
    groups, tables = _case(R, K, S, sizes)
    assert sorted(len(groups.members(g)) for g in range(groups.G)) == sorted(sizes) and groups.max_size == max(sizes)
    lo, n = R // 3, max(1, R // 2)
    for t, (T, nan_cols) in enumerate(tables):
        for min_ranks, min_peers in ((1, 1), (4, 2), (1, 2), (4, 1)):
            tag = (R, K, S, t, min_ranks, min_peers)
            got = _run(be, T, K, S, groups, 0, R, min_ranks, min_peers)
            exp = _expected(T, K, S, groups.host, groups.G, groups.max_size, 0, R, min_ranks, min_peers, 0.02)
            _compare(_flat(got), _flat(exp), tag, nan_cols)
        pcols, psc = _run(be, T, K, S, groups, lo, n, 4, 1)
        assert np.array_equal(pcols, got[0]) and np.array_equal(_bits(psc), _bits(got[1][lo : lo + n])), (R, K, S, t, "window")


@pytest.mark.parametrize("R", [8, 64, 65, 1025])
def test_one_group_and_one_peer_minimum_is_the_job_wide_robust_score(be, R):
    from nvrx_straggler.backend import PeerGroups

    K, S = 5, 3
    groups = PeerGroups([0] * R)
    T = _random_table(np.random.default_rng(R), R, K, S)
    _special(T, np.random.default_rng(R + 1), 1, "repeated", K, S)
    _special(T, np.random.default_rng(R + 2), K + 1, "equal", K, S)
    for min_ranks in (1, 4):
        gcols, gsc = _run(be, T, K, S, groups, 0, R, min_ranks, 1)
        ws = be.workspace(R, K, S, R, 0)
        cols, sc = be.robust_score(ws, ws.send, 0, R, min_ranks, 0.02).records()
        assert np.array_equal(gcols[0], cols) and np.array_equal(_bits(gsc), _bits(sc)), (R, min_ranks)


def test_out_of_range_group_contents_are_guarded(be):
    """Valid launches: the restatement's result for the clamped data, no word outside NVRX_ROBUST_GROUP_WORDS touched."""
    from nvrx_straggler import _native
    from nvrx_straggler.backend import PeerGroups

    rng = np.random.default_rng(83)
    # packed (groups of 5 or 6 in SLOT 8, and cut to 4 in SLOT 4) and 256 threads (groups of 66 and 4, cut to 65)
    for R, K, S, labels, largest in ((21, 5, 70, [r % 4 for r in range(21)], 6), (21, 5, 70, [r % 4 for r in range(21)], 4),
                                     (70, 66, 3, [1 if r % 17 == 3 else 0 for r in range(70)], 65)):
        G, KS = max(labels) + 1, K + S
        T = _random_table(rng, R, K, S)
        good = PeerGroups(labels).host
        edits = {"intact": {}, "group id G and -1": {3: G, 8: -1}, "member R and -1": {R + 2: R, R + 9: -1},
                 "start beyond R": {2 * R + G: R + 5}, "start below 0 and descending": {2 * R: -3, 2 * R + 1: 0},
                 "everything": {0: G + 7, 2 * R - 1: 1 << 30, 2 * R + G: 1 << 30, 2 * R + 1: -(1 << 30)}}
        table = torch.from_numpy(T).cuda()
        for name, edit in edits.items():
            arrays = good.copy()
            arrays[list(edit)] = list(edit.values())
            for first, n in ((0, R), (4, 9)):
                words = _native.robust_group_words(G, n, K, S)
                out = torch.full((PAD + words + PAD,), FILL, dtype=torch.int32, device="cuda")
                d_groups = torch.from_numpy(arrays).cuda()
                torch.cuda.synchronize()
                rc = be.lib.nvrx_robust_group_score(table.data_ptr(), R, K, S, d_groups.data_ptr(), G, largest, first, n, 4, 2,
                                                    0.02, out.data_ptr() + 4 * PAD, be._stream_handle)
                assert rc == 0, (name, be.lib.nvrx_last_error())
                be.synchronize()
                torch.cuda.synchronize()
                host = out.cpu().numpy().view(np.uint32)
                assert (host[:PAD] == FILL).all() and (host[PAD + words :] == FILL).all(), (R, name)
                body = host[PAD : PAD + words]
                got = (body[: 4 * G * KS].reshape(-1, 4), body[4 * G * KS :].view(np.float32).reshape(n, 2, 1 + S))
                _compare(got, _flat(_expected(T, K, S, arrays, G, largest, first, n, 4, 2, 0.02)), (R, largest, name, first, n))


@pytest.mark.parametrize("asynchronous", [False, True])
def test_through_the_public_interface(be, asynchronous):
    """The example's scenario through ``FoldedJob``; the report step equals ``backend.robust_group_score`` on the same table."""
    from nvrx_straggler.folded import FoldedJob

    names = [f"section_{s:03d}" for s in range(64)]
    rng = np.random.default_rng(2026)
    med = np.where(np.arange(8) >= 4, 1500.0, 1000.0)[:, None] * (1.0 + 0.01 * rng.standard_normal((8, 64)))
    med[6] *= 1.4
    med[4] *= 0.6
    med = med.astype(np.float32)

    def named(found):
        return sorted({s.rank for v in found.values() for group in (v.values() if isinstance(v, dict) else [v]) for s in group})

    for grouped in (True, False):
        job = FoldedJob(total_ranks=8, section_names=names, ring_cap=256, scores_to_compute=("relative_perf_scores",),
                        robust_scores=True, peer_groups="block:4", robust_peer_groups=grouped, asynchronous=asynchronous)
        try:
            fused = []
            for _ in range(3):
                for lr, r in enumerate(job.logical_ranks()):
                    job.load(lr, np.repeat(med[r][:, None], 33, axis=1))
                rep = job.report()
                t = rep.robust_scores()
                fused.append(getattr(job.reporter, "_last_plan_fused", None))
                if not grouped:
                    assert "peer_groups" not in t and named(rep.identify_robust_stragglers()) == [5, 6, 7]
                    assert t["section_center"][names[0]] == float(np.sort(med[:, 0])[3])
                    continue
                assert named(rep.identify_robust_stragglers()) == [6]
                assert t["peer_groups"] is True and t["min_peers"] == 2 and t["min_ranks"] == 4 and t["floor"] == 0.02
                assert t["groups"] == {0: [0, 1, 2, 3], 1: [4, 5, 6, 7]} and t["unrated_ranks"] == [] and t["group_of"] == {r: r // 4 for r in range(8)}
                assert t["section_center"][names[0]] == {g: float(np.sort(med[4 * g : 4 * g + 4, 0])[1]) for g in (0, 1)}
                assert t["ranks_with_data"][names[0]] == {0: 4, 1: 4}
                t["groups"][0].append(99)  # (a caller's edit of its copy does not reach the report)
                assert rep.robust_scores()["groups"][0] == [0, 1, 2, 3]
                plan = job.reporter._ring_plan
                ws = plan.ws
                be.synchronize()
                torch.cuda.synchronize()
                groups = job.reporter._peer_for(ws)
                cols, sc = be.robust_group_score(ws, ws.table, groups, 0, ws.R, 4, 2, 0.02).records()
                f = cols.view(np.float32)
                for name, c in plan.view.cols.items():
                    assert t["section_center"][name] == {g: float(f[g, ws.K + c, 0]) for g in (0, 1)}
                    assert t["section_spread"][name] == {g: float(f[g, ws.K + c, 2]) for g in (0, 1)}
                    for r in range(8):
                        assert t["section_z"][name][r] == float(sc[r, 1, 1 + c]) and t["section_ratio"][name][r] == float(sc[r, 0, 1 + c])
            assert fused == [False, True, True], fused
        finally:
            job.close()
