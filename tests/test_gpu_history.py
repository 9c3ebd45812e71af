"""The score history on the HIP engine: ``k_score_history`` through the C ABI against the NumPy restatement
(tests/history_oracle_backend.py ``history_step``), and through the engine against the CPU oracle backend.

Every word of a record is an actual score or a count and the ring holds scores as they were written, so records AND the whole
ring are compared bit for bit after every step; no tolerance is involved anywhere.

Shapes: the full cross product of H either side of each ring stride (16 | 17, 32 | 33) and at both ends (2, 64); 1 + S either
side of the four slots a wave takes at stride 16 (S = 3 | 4), either side of a whole number of waves and workgroups at every
stride (S = 63 | 64), and the smallest (0, 1); one rank, two, and 65 (an odd number of waves: the last workgroup is partly
idle); always first_rank != 0, R > n_ranks, S_cap > S.  Each case appends 2H + 3 reports one by one: the ring wraps twice.

Values: per cell a two-state chain (below its threshold / not) whose end is drawn so that four cells in five end on a streak
of 1 .. H - 1; one score column is NaN throughout; four cells carry the planted patterns.  The three smallest shapes have
fewer than five free cells ((S, n_ranks) = (0, 1), (0, 2), (1, 1): one, two and three): they take as many plants, in the order
listed in ``_sequence``, as leave one drawn cell.  Non-vacuity is asserted on the restatement's records of the LAST step (while
the ring fills, depth 1 admits no streak strictly between 0 and the depth), before the GPU is asked."""
import ctypes
import itertools

import numpy as np
import pytest

import row_family_script as script
from history_oracle_backend import CountingHistoryBackend, HistoryOracleBackend, fresh, history_step

pytestmark = pytest.mark.gpu

THRESHOLDS = (0.75, 0.7, 0.8, 0.75)  # gpu_rel, section_rel, gpu_indiv, section_indiv: all four differ from their neighbours
FIRST_RANK, EXTRA_ROWS, EXTRA_CAP = 3, 2, 3
DEPTHS, SECTIONS, RANKS = (2, 8, 16, 17, 32, 33, 64), (0, 1, 3, 4, 63, 64), (1, 2, 65)
CASES = list(itertools.product(DEPTHS, SECTIONS, RANKS))


def _column_threshold(S):
    thr = np.empty(2 + 2 * S)
    thr[0], thr[1], thr[2 : 2 + S], thr[2 + S :] = THRESHOLDS[2], THRESHOLDS[0], THRESHOLDS[3], THRESHOLDS[1]
    return thr


def _sequence(H, S, n_ranks):
    """``([2H + 3, R, 2 + 2S]`` f32 scores in [0.5, 1], number of planted cells)``: per cell a two-state chain (below its
    threshold / not), its end overwritten so that four cells in five end on a streak of 1 .. H - 1; then the NaN column and
    the planted cells."""
    rng = np.random.default_rng([H, S, n_ranks])
    steps, R, W = 2 * H + 3, FIRST_RANK + n_ranks + EXTRA_ROWS, 2 + 2 * S
    thr = _column_threshold(S)[None, :]
    below = np.empty((steps, R, W), dtype=bool)
    below[0] = rng.random((R, W)) < 0.6
    for n in range(1, steps):
        u = rng.random((R, W))
        below[n] = np.where(below[n - 1], u >= 0.5, u < 0.8)  # leaves "below" with 0.5, enters it with 0.8
    nan_col = 2 if S >= 1 else 0
    cells = [(FIRST_RANK + r, c) for c in range(W) if c != nan_col for r in range(n_ranks)]
    plants = min(4, len(cells) - 1)
    pick = [cells[(k * len(cells)) // 4] for k in range(4)] if plants == 4 else cells[:plants]
    assert len(set(pick)) == plants
    last = rng.integers(1, H, (R, W))                               # the streak the cell ends on ...
    for r, c in [cell for cell in cells if cell not in pick][4::5]:
        last[r, c] = 0                                              # ... none for every fifth drawn cell
    back = np.arange(steps)[::-1, None, None]                       # steps before the last one
    below = np.where(back < last, True, np.where(back == last, False, below))
    u = rng.random((steps, R, W))
    x = np.where(below, 0.5 + u * (thr - 0.5) * 0.999, thr + u * (1.0 - thr)).astype(np.float32)
    n = np.arange(steps)
    x[:, :, nan_col] = np.nan                                         # a column no report has: a family that was not computed
    patterns = [
        lambda c: np.where(n % 5 == 3, np.nan, 0.6),                                            # NaN entries inside a streak
        lambda c: np.array([np.inf, 0.0, thr[0, c], 0.6, thr[0, c]], dtype=np.float32)[n % 5],  # +inf, 0.0, == threshold
        lambda c: 0.5 + 0.125 * ((n // 3) % 4),                       # runs of equal scores, the same values again later
        lambda c: (0.5 + 0.01 * (n % 7)).astype(np.float32),          # every entry below
    ]
    for (r, c), pattern in zip(pick, patterns):
        x[:, r, c] = pattern(c)
    return x, plants


def _expected(H, S, n_ranks, x):
    """The restatement on the whole sequence: per step the records and the ring, and the case's claims about itself."""
    hist = fresh(n_ranks, S + EXTRA_CAP, H)
    out = []
    for n in range(x.shape[0]):
        rec = history_step(hist, x[n], S, FIRST_RANK, n_ranks, H, n, THRESHOLDS)
        out.append((rec, hist.view(np.uint32).copy()))
    return out


@pytest.fixture(scope="module")
def lib():
    import torch

    from nvrx_straggler import _native

    assert torch.cuda.is_available()
    return _native.load()


@pytest.mark.parametrize("H,S,n_ranks", CASES, ids=[f"H{h}-S{s}-n{n}" for h, s, n in CASES])
def test_the_kernel_equals_the_restatement_bit_for_bit_after_every_step(lib, H, S, n_ranks):
    import torch

    from nvrx_straggler import _native

    x, plants = _sequence(H, S, n_ranks)
    want = _expected(H, S, n_ranks, x)
    # non-vacuity, on the oracle's output, before the GPU is asked
    rec = want[-1][0]
    streak, present, depth = rec[..., 4].astype(np.int64), rec[..., 6], rec[..., 7]
    assert (depth == H).all() and ((streak > 0) & (streak < depth)).mean() >= 0.25, ((streak > 0) & (streak < depth)).mean()
    assert (present < depth).any() and (present == 0).any() and ((streak == depth).any() or plants < 4)
    assert any((r[..., 6] < r[..., 7]).any() for r, _ in want[:H])  # while the ring fills, too

    S_cap, R = S + EXTRA_CAP, x.shape[1]
    d_x = torch.from_numpy(x).cuda()
    d_hist = torch.full((_native.history_floats(n_ranks, S_cap, H) * 4,), 0xFF, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(_native.history_words(n_ranks, S), dtype=torch.int32, device="cuda")
    thr = (ctypes.c_double * 4)(*THRESHOLDS)
    stream = torch.cuda.current_stream().cuda_stream
    shape = (n_ranks, 2, 1 + S_cap, _native.history_stride(H))
    for n in range(x.shape[0]):
        d_out.fill_(-1)
        rc = lib.nvrx_score_history(d_x[n].data_ptr(), R, S, FIRST_RANK, n_ranks, d_hist.data_ptr(), S_cap, H, n, thr,
                                    d_out.data_ptr(), stream)
        assert rc == 0, lib.nvrx_last_error()
        got = d_out.cpu().numpy().view(np.uint32).reshape(n_ranks, 2, 1 + S, 8)
        ring = d_hist.cpu().numpy().view(np.uint32).reshape(shape)
        want_rec, want_ring = want[n]
        if not np.array_equal(got, want_rec):
            bad = np.argwhere((got != want_rec).any(-1))[0]
            raise AssertionError((n, tuple(bad), got[tuple(bad)].tolist(), want_rec[tuple(bad)].tolist()))
        assert np.array_equal(ring, want_ring), (n, np.argwhere(ring != want_ring)[:4].tolist())


def test_default_thresholds_are_three_quarters_each(lib):
    import torch

    H, S, n = 8, 2, 2
    x = np.array([[0.75, 0.7499999, 0.5, 0.75, 0.76, 0.1]] * n, dtype=np.float32)
    hist = fresh(n, S, H)
    want = history_step(hist, x, S, 0, n, H, 0, None)
    d_hist = torch.full((hist.size * 4,), 0xFF, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(want.size, dtype=torch.int32, device="cuda")
    rc = lib.nvrx_score_history(torch.from_numpy(x).cuda().data_ptr(), n, S, 0, n, d_hist.data_ptr(), S, H, 0, None,
                                d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.nvrx_last_error()
    got = d_out.cpu().numpy().view(np.uint32).reshape(want.shape)
    assert np.array_equal(got, want) and got[0, :, :, 4].tolist() == [[0, 1, 0], [1, 0, 1]]


def test_report_history_needs_a_report_issued_through_the_descriptor(lib):
    import torch

    from nvrx_straggler import _native
    from nvrx_straggler.backend import get_backend

    be = get_backend()
    rings = be.make_rings(1, 4, 64)
    try:
        desc = _native.ReportDesc()  # a descriptor no report went through, on a live context
        desc.R, desc.K, desc.S = 2, 0, 3
        d_hist = torch.full((_native.history_floats(2, 3, 8) * 4,), 0xFF, dtype=torch.uint8, device=be.device)
        d_out = torch.zeros(_native.history_words(2, 3), dtype=torch.int32, device=be.device)
        be.synchronize()
        torch.cuda.synchronize()
        rc = lib.nvrx_report_history(rings.ctx, ctypes.byref(desc), 0, 2, d_hist.data_ptr(), 3, 8, 0, None, d_out.data_ptr())
        assert rc == _native.ERR_STATE == -1 and b"no report was issued" in lib.nvrx_last_error()
        torch.cuda.synchronize()
        assert (d_hist.cpu().numpy() == 0xFF).all() and not d_out.cpu().numpy().any()  # nothing was launched
    finally:
        rings.close()


# ---- through the engine ---------------------------------------------------------------------------------------------------------
WINDOWS, STEP_FROM = 12, 4
OPTIONS = dict(score_history=8, persistence_min_reports=3)


def _fill(rings, rows, window):
    """tests/row_family_script.py's window, its step planted from window ``STEP_FROM`` on: rank 1's ``step`` row is flat
    before, steps up 2 x within that window, and stays up afterwards."""
    for (name, lr), values in script.pushes(window).items():
        if (name, lr) == ("step", 1):
            flat = script.pushes(window)[("step", 0)]
            values = flat if window < STEP_FROM else values if window == STEP_FROM else np.float32(2.0) * flat
        rings.push_many(rows[name], values, lr=lr)


def _run(be, asynchronous, **options):
    """``WINDOWS`` reports, unread until all were issued: per report its path, history, persistent stragglers, the raw
    records and the device flags."""
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=True, node_name="n",
                          asynchronous=asynchronous, **options)
    rings = be.make_rings(script.LOCAL_RANKS, len(script.ROWS), script.RING_CAP)
    rows = {name: rings.row_for(0, name) for name in script.ROWS}
    reports, planned = [], []
    try:
        for w in range(WINDOWS):
            _fill(rings, rows, w)
            planned.append(gen._ring_plan is not None)
            reports.append(gen.generate_report_from_rings(rings, rows, {}, local_ranks=script.LOCAL_RANKS))
            rings.reset()
        out = []
        for rep, was_planned in zip(reports, planned):
            src = rep.__dict__.get("_history")
            out.append({"planned": was_planned, "records": None if src is None else np.array(src.handle.records()),
                        "cols": None if src is None else dict(src.sections), "flags": np.array(rep._flags()._array()),
                        "history": rep.score_history(), "persistent": rep.identify_persistent_stragglers(),
                        "stragglers": rep.identify_stragglers()})
        return out, gen
    finally:
        gen.close()
        close = getattr(rings, "close", None)
        if close is not None:
            close()


@pytest.fixture(scope="module")
def oracle_runs():
    """The reference, computed once: the same windows on the CPU oracle backend."""
    from nvrx_straggler import backend

    before, cpu = backend._backend, HistoryOracleBackend()
    backend.set_backend(cpu)
    try:
        return _run(cpu, False, **OPTIONS)[0]
    finally:
        backend.set_backend(before)


@pytest.mark.parametrize("asynchronous", [False, True], ids=["synchronous", "asynchronous"])
def test_the_engine_keeps_the_oracles_history_on_the_general_and_the_planned_path(oracle_runs, asynchronous):
    from nvrx_straggler.backend import get_backend

    got, _ = _run(get_backend(), asynchronous, **OPTIONS)
    assert [e["planned"] for e in got] == [False] + [True] * (WINDOWS - 1)  # the general path once, then the cached plan
    S = len(script.ROWS)
    for w, (g, o) in enumerate(zip(got, oracle_runs)):
        assert script.same(g["history"], o["history"]), (w, g["history"], o["history"])
        assert g["persistent"] == o["persistent"] and g["stragglers"] == o["stragglers"], w
        assert g["history"]["depth"] == min(w + 1, 8)
        # rank 1 is flagged on "step" from the window after its step on, and persistently two reports later
        flagged = {s.rank for s in g["persistent"]["straggler_sections_relative"].get("step", ())}
        assert flagged == ({1} if w >= STEP_FROM + 3 else set()), (w, g["persistent"])
        assert g["history"]["section_relative"]["step"][1]["streak"] == max(0, w - STEP_FROM)
        # streak > 0 exactly where the report's own device flag is set
        rec, flags = g["records"], g["flags"]
        for f in (0, 1):
            cols = [f] + [2 + f * S + j for j in range(S)]
            assert np.array_equal(rec[:, f, :, 4] > 0, flags[:, cols] != 0), (w, f, rec[:, f, :, 4], flags[:, cols])
    assert any(e["flags"].any() for e in got) and not all(e["flags"].all() for e in got)


@pytest.mark.parametrize("asynchronous", [False, True], ids=["synchronous", "asynchronous"])
def test_with_the_option_off_a_report_makes_no_history_call(asynchronous):
    from nvrx_straggler.backend import get_backend

    be = get_backend()
    calls = []
    saved = {name: getattr(be, name) for name in ("score_history", "history_prepare", "history_copy_out")}
    saved_lib = {name: getattr(be.lib, name) for name in ("nvrx_score_history", "nvrx_report_history")}

    def spy(name, inner):
        def call(*a, **kw):
            calls.append(name)
            return inner(*a, **kw)

        return call

    for name, inner in saved.items():
        setattr(be, name, spy(name, inner))
    for name, inner in saved_lib.items():
        setattr(be.lib, name, spy(name, inner))
    try:
        off, gen = _run(be, asynchronous)
        assert calls == [] and gen._history is None
        assert all(e["history"] == {} and e["records"] is None for e in off)
        ws = gen._ring_plan.ws if gen._ring_plan is not None else None
        assert ws is None or ws._history_last is None  # (workspaces are shared by shape: only what is in flight is this run's)
        on, _ = _run(be, asynchronous, **OPTIONS)
        steps = [c for c in calls if c.startswith("nvrx_")]
        assert len(steps) == WINDOWS and calls.count("history_copy_out") == WINDOWS  # one launch and one copy-out per report
        # ... and what a report says besides is the same either way
        for a, b in zip(off, on):
            assert a["stragglers"] == b["stragglers"] and np.array_equal(a["flags"], b["flags"])
    finally:
        for name, inner in saved.items():
            setattr(be, name, inner)
        for name, inner in saved_lib.items():
            setattr(be.lib, name, inner)
    # the CPU checker that only counts: the generator's paths never reach for the history either
    from nvrx_straggler import backend

    before, counting = backend._backend, CountingHistoryBackend(emulate_fused=True)
    backend.set_backend(counting)
    try:
        _run(counting, asynchronous)
        assert counting.history_calls == 0
    finally:
        backend.set_backend(before)
