"""The peer-score history and trends on the HIP engine: ``k_peer_history`` / ``k_peer_trend`` through the C ABI against the
restatement (tests/peer_history_oracle_backend.py: ``history_step`` / ``trend_records`` on the embedded peer plane, family 1) and
against ``nvrx_score_history`` / ``nvrx_score_trend`` on the same embedding ON THE DEVICE, and through the engine against the
CPU oracle backend.

Every word of a record is an actual score, a count, or one correctly rounded f64 operation, and the ring holds scores as they
were written: records AND whole rings are compared bit for bit after every step; no tolerance is involved anywhere.

Shapes: H at both ends and either side of each ring stride (2, 16 | 17, 32 | 33, 64); 1 + S either side of the four slots a
wave takes at stride 16 (S = 3 | 4), either side of whole waves and workgroups (S = 63 | 64), and the GPU slot alone (S = 0);
one rank, two, and 65 (an odd number of waves: the last workgroup is partly idle); S_cap = S + 3.  Each case appends 2H + 3
reports one by one: the ring wraps twice.

Values, as tests/test_gpu_history.py draws them: per cell a two-state chain (below its threshold / not) whose end is drawn so
that four drawn cells in five end on a streak of 1 .. H - 1; slot 1 is NaN throughout where S >= 1 (with S = 0 and more than two
ranks: one rank's cell); four cells carry the planted patterns.  S = 0 with one or two ranks has one or two cells: they take as
many plants as leave one drawn cell and no all-NaN cell.  Non-vacuity is asserted on the restatement's records of the LAST
step, before the GPU is asked.

The trend restatement sorts every cell's H (H - 1) / 2 pair slopes.  ``nvrx_peer_trend`` is compared with ``nvrx_score_trend``
(device against device, and the ring's bytes before and after) after EVERY step of every shape; with the restatement after
every step where cells x pairs <= ``EVERY_STEP_WORK``, and after steps 1, 2, 3, H - 1, H, H + 1 and the last in the heavier
shapes (tests/test_gpu_trend.py's rule: it keeps a case within a few seconds)."""
import ctypes
import functools
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import peer_history_workers as workers
import row_family_script as script
from mp_util import run_ranks
from peer_history_oracle_backend import (PeerHistoryOracleBackend, embed, peer_fresh, peer_history_step, peer_trend_records)

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THRESHOLDS = (0.75, 0.7)  # gpu, section
SCORE_THRESHOLDS = (0.75, 0.7, 0.8, 0.75)  # the embedding's: the relative pair is THRESHOLDS
EXTRA_CAP, GUARD = 3, 16
DEPTHS, SECTIONS, RANKS = (2, 16, 17, 32, 33, 64), (0, 3, 4, 63, 64), (1, 2, 65)
CASES = list(itertools.product(DEPTHS, SECTIONS, RANKS))
IDS = [f"H{h}-S{s}-n{n}" for h, s, n in CASES]
EVERY_STEP_WORK = 300_000  # cells x pairs per step of the trend restatement


def _sequence(H, S, n_ranks):
    """``([2H + 3, n_ranks, 1 + S]`` f32 peer scores in [0.5, 1], number of planted cells)``."""
    rng = np.random.default_rng([11, H, S, n_ranks])
    steps, W = 2 * H + 3, 1 + S
    thr = np.array([THRESHOLDS[0]] + [THRESHOLDS[1]] * S)[None, :]
    below = np.empty((steps, n_ranks, W), dtype=bool)
    below[0] = rng.random((n_ranks, W)) < 0.6
    for n in range(1, steps):
        u = rng.random((n_ranks, W))
        below[n] = np.where(below[n - 1], u >= 0.5, u < 0.8)  # leaves "below" with 0.5, enters it with 0.8
    absent = np.zeros((n_ranks, W), dtype=bool)
    if S >= 1:
        absent[:, 1] = True          # a section no rank is ever rated on
    elif n_ranks > 2:
        absent[0, 0] = True          # a rank that never has a peer
    cells = [(r, c) for c in range(W) for r in range(n_ranks) if not absent[r, c]]
    plants = min(4, len(cells) - 1)
    pick = [cells[(k * len(cells)) // 4] for k in range(4)] if plants == 4 else cells[:plants]
    assert len(set(pick)) == plants
    last = rng.integers(1, H, (n_ranks, W))                         # the streak the cell ends on ...
    for r, c in [cell for cell in cells if cell not in pick][4::5]:
        last[r, c] = 0                                              # ... none for every fifth drawn cell
    back = np.arange(steps)[::-1, None, None]                       # steps before the last one
    below = np.where(back < last, True, np.where(back == last, False, below))
    u = rng.random((steps, n_ranks, W))
    x = np.where(below, 0.5 + u * (thr - 0.5) * 0.999, thr + u * (1.0 - thr)).astype(np.float32)
    n = np.arange(steps)
    x[:, absent] = np.nan
    patterns = [
        lambda c: np.where(n % 5 == 3, np.nan, 0.6),                                            # NaN inside a streak: unrated now and then
        lambda c: np.array([np.inf, 0.0, thr[0, c], 0.6, thr[0, c]], dtype=np.float32)[n % 5],  # +inf, 0.0, == threshold
        lambda c: 0.5 + 0.125 * ((n // 3) % 4),                       # runs of equal scores, the same values again later
        lambda c: (0.5 + 0.01 * (n % 7)).astype(np.float32),          # every entry below
    ]
    for (r, c), pattern in zip(pick, patterns):
        x[:, r, c] = pattern(c)
    return x, plants


@functools.lru_cache(maxsize=2)
def _expected(H, S, n_ranks):
    """The sequence and the restatement on it: per step the records and the ring; the case's claims about itself asserted."""
    x, plants = _sequence(H, S, n_ranks)
    hist = peer_fresh(n_ranks, S + EXTRA_CAP, H)
    out = []
    for n in range(x.shape[0]):
        rec = peer_history_step(hist, x[n], S, H, n, THRESHOLDS)
        out.append((rec, hist.view(np.uint32).copy()))
    # non-vacuity, on the restatement's last-step records, before the GPU is asked
    rec = out[-1][0]
    streak, present, depth = rec[..., 4].astype(np.int64), rec[..., 6], rec[..., 7]
    assert (depth == H).all()
    if n_ranks * (1 + S) >= 6:
        inside = (streak > 0) & (streak < depth)
        assert inside.mean() >= 0.25, inside.mean()
        assert (present < depth).any() and (present == 0).any()
    return x, out


@pytest.fixture(scope="module")
def lib():
    import torch

    from nvrx_straggler import _native

    assert torch.cuda.is_available()
    return _native.load()


def _device_state(n_ranks, S, H):
    import torch

    from nvrx_straggler import _native

    S_cap = S + EXTRA_CAP
    peer_ring = torch.full((_native.peer_history_floats(n_ranks, S_cap, H) * 4,), 0xFF, dtype=torch.uint8, device="cuda")
    score_ring = torch.full((_native.history_floats(n_ranks, S_cap, H) * 4,), 0xFF, dtype=torch.uint8, device="cuda")
    return S_cap, peer_ring, score_ring


# ---- 1 + 2. nvrx_peer_history against the restatement, and against nvrx_score_history on the embedded plane -------------------
@pytest.mark.parametrize("H,S,n_ranks", CASES, ids=IDS)
def test_the_history_kernel_equals_the_restatement_and_family_one_of_the_score_history_after_every_step(lib, H, S, n_ranks):
    import torch

    from nvrx_straggler import _native

    x, want = _expected(H, S, n_ranks)
    S_cap, d_ring, d_ring2 = _device_state(n_ranks, S, H)
    Hs = _native.history_stride(H)
    d_x = torch.from_numpy(x).cuda()
    d_rows = torch.from_numpy(np.stack([embed(x[n], S) for n in range(x.shape[0])])).cuda()  # [steps, n_ranks, 2 + 2S]
    words = _native.peer_history_words(n_ranks, S)
    d_out = torch.zeros(words + GUARD, dtype=torch.int32, device="cuda")
    d_out2 = torch.zeros(_native.history_words(n_ranks, S), dtype=torch.int32, device="cuda")
    thr, thr4 = (ctypes.c_double * 2)(*THRESHOLDS), (ctypes.c_double * 4)(*SCORE_THRESHOLDS)
    stream = torch.cuda.current_stream().cuda_stream
    for n in range(x.shape[0]):
        d_out.fill_(-1)
        rc = lib.nvrx_peer_history(d_x[n].data_ptr(), n_ranks, S, d_ring.data_ptr(), S_cap, H, n, thr, d_out.data_ptr(), stream)
        assert rc == 0, lib.nvrx_last_error()
        rc = lib.nvrx_score_history(d_rows[n].data_ptr(), n_ranks, S, 0, n_ranks, d_ring2.data_ptr(), S_cap, H, n, thr4,
                                    d_out2.data_ptr(), stream)
        assert rc == 0, lib.nvrx_last_error()
        host = d_out.cpu().numpy().view(np.uint32)
        got = host[:words].reshape(n_ranks, 1, 1 + S, 8)
        ring = d_ring.cpu().numpy().view(np.uint32).reshape(n_ranks, 1 + S_cap, Hs)
        want_rec, want_ring = want[n]
        if not np.array_equal(got, want_rec):
            bad = np.argwhere((got != want_rec).any(-1))[0]
            raise AssertionError((n, tuple(bad), got[tuple(bad)].tolist(), want_rec[tuple(bad)].tolist()))
        assert np.array_equal(ring, want_ring), (n, np.argwhere(ring != want_ring)[:4].tolist())
        assert (host[words:] == 0xFFFFFFFF).all()  # nothing behind the records
        # the same definition on the device: family 1 of the score history on the embedded rows
        got2 = d_out2.cpu().numpy().view(np.uint32).reshape(n_ranks, 2, 1 + S, 8)
        ring2 = d_ring2.cpu().numpy().view(np.uint32).reshape(n_ranks, 2, 1 + S_cap, Hs)
        assert np.array_equal(got2[:, 1], got[:, 0]), (n, np.argwhere((got2[:, 1] != got[:, 0]).any(-1))[:4].tolist())
        assert np.array_equal(ring2[:, 1], ring), n


def test_default_thresholds_are_three_quarters_each(lib):
    import torch

    n, S, H = 2, 2, 8
    x = np.array([[0.7499999, 0.75, 0.1]] * n, dtype=np.float32)
    hist = peer_fresh(n, S, H)
    want = peer_history_step(hist, x, S, H, 0, None)
    d_ring = torch.full((hist.size * 4,), 0xFF, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(want.size, dtype=torch.int32, device="cuda")
    rc = lib.nvrx_peer_history(torch.from_numpy(x).cuda().data_ptr(), n, S, d_ring.data_ptr(), S, H, 0, None, d_out.data_ptr(),
                               torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.nvrx_last_error()
    got = d_out.cpu().numpy().view(np.uint32).reshape(want.shape)
    assert np.array_equal(got, want) and got[0, 0, :, 4].tolist() == [1, 0, 1]


# ---- 3. nvrx_peer_trend against nvrx_score_trend and the trend restatement; the ring is only read -------------------------------
def _restated_steps(H, S, n_ranks):
    steps = 2 * H + 3
    if n_ranks * (1 + S) * H * (H - 1) // 2 <= EVERY_STEP_WORK:
        return set(range(1, steps + 1))
    return {1, 2, 3, H - 1, H, H + 1, steps}


@pytest.mark.parametrize("H,S,n_ranks", CASES, ids=IDS)
def test_the_trend_kernel_equals_the_score_trend_and_the_restatement_and_only_reads_the_ring(lib, H, S, n_ranks):
    import torch

    from nvrx_straggler import _native

    x, want = _expected(H, S, n_ranks)
    steps = x.shape[0]
    restated = _restated_steps(H, S, n_ranks)
    # non-vacuity, on the restatement's records of the last step, before the GPU is asked
    last = peer_trend_records(want[-1][1].view(np.float32), S, H, steps)
    usable, mk = last[..., 3].astype(np.int64), last[..., 2].view(np.int32)
    cells = n_ranks * (1 + S)
    absent = n_ranks if S >= 1 else int(n_ranks > 2)
    drawn = cells - absent - min(4, cells - absent - 1)  # (two drawn cells need not hold a rising and a falling one)
    if cells >= 6:
        assert (usable < 2).any() and (drawn < 4 or ((mk > 0).any() and (mk < 0).any()))
    S_cap, d_ring, d_ring2 = _device_state(n_ranks, S, H)
    d_x = torch.from_numpy(x).cuda()
    d_rows = torch.from_numpy(np.stack([embed(x[n], S) for n in range(steps)])).cuda()
    d_rec = torch.zeros(_native.history_words(n_ranks, S), dtype=torch.int32, device="cuda")
    words = _native.peer_trend_words(n_ranks, S)
    d_out = torch.zeros(words + GUARD, dtype=torch.int32, device="cuda")
    d_out2 = torch.zeros(_native.trend_words(n_ranks, S), dtype=torch.int32, device="cuda")
    thr, thr4 = (ctypes.c_double * 2)(*THRESHOLDS), (ctypes.c_double * 4)(*SCORE_THRESHOLDS)
    stream = torch.cuda.current_stream().cuda_stream
    for n in range(steps):
        assert lib.nvrx_peer_history(d_x[n].data_ptr(), n_ranks, S, d_ring.data_ptr(), S_cap, H, n, thr, d_rec.data_ptr(),
                                     stream) == 0, lib.nvrx_last_error()
        assert lib.nvrx_score_history(d_rows[n].data_ptr(), n_ranks, S, 0, n_ranks, d_ring2.data_ptr(), S_cap, H, n, thr4,
                                      d_rec.data_ptr(), stream) == 0, lib.nvrx_last_error()
        before = d_ring.clone()
        d_out.fill_(-1)
        assert lib.nvrx_peer_trend(d_ring.data_ptr(), n_ranks, S, S_cap, H, n + 1, d_out.data_ptr(), stream) == 0, lib.nvrx_last_error()
        assert lib.nvrx_score_trend(d_ring2.data_ptr(), n_ranks, S, S_cap, H, n + 1, d_out2.data_ptr(), stream) == 0, lib.nvrx_last_error()
        host = d_out.cpu().numpy().view(np.uint32)
        got = host[:words].reshape(n_ranks, 1, 1 + S, 4)
        got2 = d_out2.cpu().numpy().view(np.uint32).reshape(n_ranks, 2, 1 + S, 4)
        assert torch.equal(before, d_ring), n  # the launch left the ring's bytes alone
        assert (host[words:] == 0xFFFFFFFF).all()
        assert np.array_equal(got[:, 0], got2[:, 1]), (n, np.argwhere((got[:, 0] != got2[:, 1]).any(-1))[:4].tolist())
        if n + 1 in restated:
            ring = want[n][1].view(np.float32)
            assert np.array_equal(d_ring.cpu().numpy().view(np.uint32).reshape(ring.shape), want[n][1]), n
            want_rec = peer_trend_records(ring, S, H, n + 1)
            if not np.array_equal(got, want_rec):
                bad = np.argwhere((got != want_rec).any(-1))[0]
                raise AssertionError((n, tuple(bad), got[tuple(bad)].tolist(), want_rec[tuple(bad)].tolist()))


# ---- 4. ordering: the report forms follow the context's peer step -------------------------------------------------------------------
def test_the_report_forms_need_a_report_and_then_read_the_peer_steps_block(lib):
    import torch

    from nvrx_straggler import _native
    from nvrx_straggler.backend import PeerHistory, get_backend
    from nvrx_straggler.reporting import ReportGenerator

    be = get_backend()
    rings = be.make_rings(8, 4, 64)
    gen = None
    try:
        # a live context no report went through
        d_peer = torch.zeros(8 * 5, dtype=torch.float32, device=be.device)
        d_ring = torch.full((_native.peer_history_floats(8, 4, 8) * 4,), 0xFF, dtype=torch.uint8, device=be.device)
        d_out = torch.zeros(_native.peer_history_words(8, 4), dtype=torch.int32, device=be.device)
        be.synchronize()
        torch.cuda.synchronize()
        rc = lib.nvrx_report_peer_history(rings.ctx, d_peer.data_ptr(), 8, 4, d_ring.data_ptr(), 4, 8, 0, None, d_out.data_ptr())
        assert rc == _native.ERR_STATE == -1 and b"no report was issued" in lib.nvrx_last_error()
        rc = lib.nvrx_report_peer_trend(rings.ctx, d_ring.data_ptr(), 8, 4, 4, 8, 1, d_out.data_ptr())
        assert rc == _native.ERR_STATE and b"no report was issued" in lib.nvrx_last_error()
        torch.cuda.synchronize()
        assert (d_ring.cpu().numpy() == 0xFF).all() and not d_out.cpu().numpy().any()  # nothing was launched
        # a report plus nvrx_report_peer: the step reads the rank part that step left in the workspace's peer slot
        gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=True, node_name="n", peer_groups="block:4")
        names = [f"section_{s:03d}" for s in range(4)]
        rows, no_kernels = {n: rings.row_for(0, n) for n in names}, {}  # (the same objects every report: the plan is kept)
        data = workers.stage_windows(3)
        for i in range(2):  # the general path, then the one-call report
            for lr in range(8):
                for s, n in enumerate(names):
                    rings.push_many(rows[n], data[i, lr, s], lr=lr)
            rep = gen.generate_report_from_rings(rings, rows, no_kernels, local_ranks=8)
            rings.reset()
        assert gen._last_plan_fused
        ws, peer = gen._ring_plan.ws, rep.__dict__["_peer"].handle
        state = PeerHistory(8)
        h = rings.report_peer_history(ws, state, peer, THRESHOLDS)
        t = rings.report_peer_trend(ws, state)
        assert state.n_before == 1 and state.ranks == (0, 8)
        scores = peer.records()[1]
        hist = peer_fresh(8, 64, 8)
        assert np.array_equal(h.records(), peer_history_step(hist, scores, 4, 8, 0, THRESHOLDS))
        assert np.array_equal(t.records(), peer_trend_records(hist, 4, 8, 1))
        assert np.array_equal(state.hist.cpu().numpy().view(np.uint32), hist.view(np.uint32))
        assert (scores[:, 1:] < 1.0).any() and np.isnan(scores[:, 0]).all()  # (no kernels: the GPU slot is unrated)
    finally:
        if gen is not None:
            gen.close()
        rings.close()


# ---- 5. through the engine, against the oracle backend ------------------------------------------------------------------------------
REPORTS = 12
OPTIONS = dict(peer_history=8, peer_persistence_min_reports=3, peer_trends=True, trend_min_reports=4)


@pytest.fixture(scope="module", params=["block:4", "auto"])
def oracle_runs(request):
    """The reference, computed once per way of naming the groups: the same reports on the CPU oracle backend."""
    from nvrx_straggler import backend

    before, cpu = backend._backend, PeerHistoryOracleBackend()
    backend.set_backend(cpu)
    try:
        return request.param, workers.folded_reports(0, 1, reports=REPORTS, peer_groups=request.param, **OPTIONS)
    finally:
        backend.set_backend(before)


@pytest.mark.parametrize("asynchronous", [False, True], ids=["synchronous", "asynchronous"])
def test_the_engine_keeps_the_oracles_peer_history_on_the_general_and_the_planned_path(oracle_runs, asynchronous):
    peer_groups, want = oracle_runs
    got = workers.folded_reports(0, 1, reports=REPORTS, peer_groups=peer_groups, asynchronous=asynchronous, **OPTIONS)
    assert [e["planned"] for e in got] == [False] + [True] * (REPORTS - 1)  # the general path once, then the cached plan
    name = "section_000"
    for w, (g, o) in enumerate(zip(got, want)):
        assert script.same(g["peer_history"], o["peer_history"]), (w, g["peer_history"], o["peer_history"])
        assert script.same(g["peer_trends"], o["peer_trends"]), (w, g["peer_trends"], o["peer_trends"])
        assert g["persistent"] == o["persistent"] and g["declining"] == o["declining"] and g["per_report"] == o["per_report"], w
        assert np.array_equal(g["records"], o["records"]), w
        assert g["peer_history"]["depth"] == min(w + 1, 8) == g["peer_trends"]["depth"]
        # (named or inferred, the groups are the two stages)  rank 6 is slower than its stage from report 4 on: named per
        # report at once, persistently two reports later; rank 1's one bad window (report 2) is named per report and never
        # persistently; the faster stage does not have the last section and is unrated on it throughout
        assert g["per_report"] == ([1] if w == 2 else [6] if w >= 4 else []), (w, g["per_report"])
        named = {s for v in g["persistent"]["straggler_sections_relative"].values() for s in v}
        assert named == ({6} if w >= 6 else set()), (w, g["persistent"])
        assert g["peer_history"]["section_relative"][name][6]["streak"] == max(0, w - 3)
        assert g["peer_history"]["section_relative"]["section_004"][0]["present"] == 0
        assert g["peer_history"]["section_relative"]["section_004"][5]["present"] == min(w + 1, 8)
    assert any(e["persistent"]["straggler_sections_relative"] for e in got)


@pytest.mark.parametrize("asynchronous", [False, True], ids=["synchronous", "asynchronous"])
def test_with_the_option_off_a_report_makes_no_peer_history_call(asynchronous):
    from nvrx_straggler.backend import get_backend

    be = get_backend()
    calls = []
    names = ("nvrx_peer_history", "nvrx_report_peer_history", "nvrx_peer_trend", "nvrx_report_peer_trend")
    saved = {name: getattr(be.lib, name) for name in names}

    def spy(name, inner):
        def call(*a, **kw):
            calls.append(name)
            return inner(*a, **kw)

        return call

    for name, inner in saved.items():
        setattr(be.lib, name, spy(name, inner))
    try:
        off = workers.folded_reports(0, 1, reports=4, asynchronous=asynchronous)
        assert calls == [] and all(e["peer_history"] == {} and e["peer_trends"] == {} and e["records"] is None for e in off)
        on = workers.folded_reports(0, 1, reports=4, asynchronous=asynchronous, **OPTIONS)
        assert sorted(set(calls)) == ["nvrx_peer_history", "nvrx_peer_trend", "nvrx_report_peer_history", "nvrx_report_peer_trend"]
        assert len(calls) == 8  # one history and one trend launch per report
        for a, b in zip(off, on):  # what a report says besides is the same either way
            assert a["per_report"] == b["per_report"] and script.same(a["peer_section_relative"], b["peer_section_relative"])
    finally:
        for name, inner in saved.items():
            setattr(be.lib, name, inner)


# ---- 6. four processes sharing the GPU ------------------------------------------------------------------------------------------------
def test_four_processes_sharing_the_gpu_keep_the_oracles_records_each_for_its_own_rank():
    from nvrx_straggler import backend

    options = dict(reports=6, total_ranks=4, peer_groups="mod:2", peer_history=4, peer_persistence_min_reports=2)
    before, cpu = backend._backend, PeerHistoryOracleBackend()
    backend.set_backend(cpu)
    try:
        want = workers.folded_reports(0, 1, **options)
    finally:
        backend.set_backend(before)
    res = run_ranks(workers.folded_reports, 4, timeout=420, use_oracle_backend=False, device=0, gather_on_rank0=False, **options)
    for rank in range(4):
        assert len(res[rank]) == 6
        for w, (g, o) in enumerate(zip(res[rank], want)):
            assert g["records"].shape == (1,) + o["records"].shape[1:]
            assert np.array_equal(g["records"][0], o["records"][rank]), (rank, w)
            t, ref = g["peer_history"], o["peer_history"]
            assert t["depth"] == min(w + 1, 4) == ref["depth"]
            assert sorted(t["gpu_relative"]) == [rank]
            for n, per_rank in t["section_relative"].items():
                assert sorted(per_rank) == [rank] and script.same(per_rank[rank], ref["section_relative"][n][rank]), (rank, w, n)
    assert any(res[r][w]["peer_history"]["section_relative"]["section_000"][r]["streak"] >= 2 for r in range(4) for w in range(6))


# ---- 7. the example ---------------------------------------------------------------------------------------------------------------------
def test_the_example_prints_the_three_verdict_sequences():
    out = subprocess.run([sys.executable, os.path.join(REPO, "examples", "straggler_example.py"), "--peer-persist"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = re.findall(r"report +(\d+): identify_peer_stragglers\(\) (\[[^\]]*\]), identify_persistent_stragglers\(\) (\[[^\]]*\]), "
                       r"identify_persistent_peer_stragglers\(\) (\[[^\]]*\])", out.stdout)
    assert [int(i) for i, _, _, _ in lines] == list(range(16)), out.stdout
    for i, (_, per_report, job_wide, peers) in enumerate(lines):
        assert per_report == ("[1]" if i == 6 else "[6]" if i >= 10 else "[]"), (i, per_report)
        assert job_wide == ("[4, 5, 6, 7]" if i >= 2 else "[]"), (i, job_wide)
        assert peers == ("[6]" if i >= 12 else "[]"), (i, peers)
