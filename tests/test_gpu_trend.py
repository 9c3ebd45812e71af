"""Score trends on the HIP engine: ``k_score_trend`` through the C ABI against the brute-force NumPy restatement
(tests/trend_oracle_backend.py ``trend_records``), and through the engine against the CPU oracle backend.

Every word of a record is one correctly rounded f64 operation and one conversion away from the ring's entries, or a count, so
records are compared bit for bit; no tolerance is involved anywhere.  The ring itself is driven by ``nvrx_score_history`` --
one launch per step of a sequence of 2H + 3 reports, the ring wraps twice -- and must be byte-identical before and after every
trend launch: the kernel only reads it.

Shapes: H either side of each ring stride (16 | 17, 32 | 33), equal to a stride (16, 32, 64) and below the smallest (4, 8);
1 + S either side of the four slots a wave takes at stride 16 (S = 3 | 4), either side of a whole number of waves and
workgroups at every stride (S = 63 | 64), and the smallest (0, 1); one rank, two, and 65 (an odd number of waves: the last
workgroup is partly idle); always S_cap > S.

Steps compared.  The restatement sorts every cell's H (H - 1) / 2 pair slopes, so its cost per step is cells x pairs.  Shapes
with n_ranks * 2 * (1 + S) * H (H - 1) / 2 <= ``EVERY_STEP_WORK`` are compared after EVERY step; the others -- ``SUBSET``,
17 of the 126; with the limit below: n_ranks = 65 with (H >= 16, S >= 63), (H >= 32, S = 4) or (H = 64, S >= 1), and n_ranks = 2
with H = 64 and S >= 63 -- after steps 1, 2, 3, H - 1, H, H + 1 and the last (the history kernel still runs at every step).

Values: four drawn cells in five move on a grid of 1/64 (a drift plus noise, rounded), which makes many pair slopes equal --
the median slope is then one of a run of ties --, the others are unrounded floats; one score column (with S = 0: one cell) is NaN throughout; six
cells carry the planted patterns of ``_sequence``.  The smallest shapes have fewer free cells than plants and take as many as
leave one drawn cell; a shape with fewer than eight free cells need not hold both a rising and a falling one (S = 0 with one
rank has ONE free cell).  Non-vacuity is asserted on the restatement's records of the last step, before the GPU is asked."""
import ctypes
import itertools

import numpy as np
import pytest

from history_oracle_backend import fresh, history_step
from trend_oracle_backend import CountingTrendBackend, TrendOracleBackend, aged, pair_slopes, trend_records

pytestmark = pytest.mark.gpu

THRESHOLDS = (0.75, 0.7, 0.8, 0.75)
FIRST_RANK, EXTRA_ROWS, EXTRA_CAP, GUARD = 3, 2, 3, 16
DEPTHS, SECTIONS, RANKS = (4, 8, 16, 17, 32, 33, 64), (0, 1, 3, 4, 63, 64), (1, 2, 65)
CASES = list(itertools.product(DEPTHS, SECTIONS, RANKS))
EVERY_STEP_WORK = 300_000  # cells x pairs per step: a sort of that many keys per step keeps a case within a few seconds
SUBSET = [(h, s, n) for h, s, n in CASES if n * 2 * (1 + s) * h * (h - 1) // 2 > EVERY_STEP_WORK]


def _steps_compared(H, S, n_ranks):
    steps = 2 * H + 3
    if (H, S, n_ranks) not in SUBSET:
        return list(range(1, steps + 1))
    return sorted({1, 2, 3, H - 1, H, H + 1, steps})


def _sequence(H, S, n_ranks):
    """``([2H + 3, R, 2 + 2S]`` f32 scores, number of planted cells)``."""
    rng = np.random.default_rng([7, H, S, n_ranks])
    steps, R, W = 2 * H + 3, FIRST_RANK + n_ranks + EXTRA_ROWS, 2 + 2 * S
    n = np.arange(steps)
    drift = rng.choice([-1.0, 1.0], (R, W)) * rng.uniform(0.0, 0.01, (R, W))   # rising and falling cells
    x = 0.85 + drift[None] * (n[:, None, None] - steps / 2) / 4 + 0.01 * rng.standard_normal((steps, R, W))
    on_grid = (np.arange(R)[:, None] + np.arange(W)[None, :]) % 5 != 0  # four cells in five
    x = np.where(on_grid[None], np.round(x * 64) / 64, x).astype(np.float32)
    absent = np.zeros((R, W), dtype=bool)                           # cells no report has a score for: usable == 0 ...
    if S >= 1:
        absent[:, 2] = True                                         # ... a whole column (a family that was not computed),
    else:
        absent[FIRST_RANK, 0] = True                                # or, where there are only two columns, one rank's
    x[:, absent] = np.nan
    cells = [(FIRST_RANK + r, c) for c in range(W) for r in range(n_ranks) if not absent[FIRST_RANK + r, c]]
    patterns = [
        lambda: (1.0 - n / 64.0).astype(np.float32),                                      # an exactly linear fall
        lambda: np.full(steps, 0.625, dtype=np.float32),                                  # all entries equal
        lambda: np.where(n % 2 == 0, 0.5, 0.75).astype(np.float32),                       # two alternating values: tied slopes
        lambda: np.where(n % 5 == 3, np.nan, 0.9 - 0.002 * n).astype(np.float32),         # NaN on every fifth report
        lambda: np.array([np.inf, 0.0, 0.7, 0.6, 0.65], dtype=np.float32)[n % 5],         # a +inf and a 0.0
        lambda: np.where(n % (H + 1) == H, 0.8, np.nan).astype(np.float32),               # at most one usable entry
    ]
    plants = min(len(patterns), len(cells) - 1)
    pick = [cells[(k * len(cells)) // plants] for k in range(plants)]
    assert len(set(pick)) == plants
    for (r, c), pattern in zip(pick, patterns):
        x[:, r, c] = pattern()
    return x, plants


def _tied_or_adjacent(hist, S, H, n_reports):
    """Per cell with at least two pairs: is the median pair slope one of a run of equal keys, or next to a key one apart?"""
    keys, n_pairs, _ = pair_slopes(aged(hist, S, H, n_reports))
    keys = np.sort(keys, axis=-1).astype(np.int64)
    k = np.clip((n_pairs - 1) >> 1, 0, None)
    mid = np.take_along_axis(keys, k[..., None], -1)[..., 0]
    lo = np.take_along_axis(keys, np.clip(k - 1, 0, None)[..., None], -1)[..., 0]
    hi = np.take_along_axis(keys, np.clip(k + 1, None, keys.shape[-1] - 1)[..., None], -1)[..., 0]
    near = ((k >= 1) & (mid - lo <= 1)) | ((k + 1 < n_pairs) & (hi - mid <= 1))
    return near & (n_pairs >= 2)


def _expected(H, S, n_ranks):
    """The sequence, the restatement's records ``{n_reports: records}`` at the steps compared, and the ring after the last
    step -- with the case's claims about itself asserted on them."""
    x, plants = _sequence(H, S, n_ranks)
    S_cap, steps = S + EXTRA_CAP, x.shape[0]
    compared = _steps_compared(H, S, n_ranks)
    hist = fresh(n_ranks, S_cap, H)
    want = {}
    for n in range(steps):
        history_step(hist, x[n], S, FIRST_RANK, n_ranks, H, n, THRESHOLDS)
        if n + 1 in compared:
            want[n + 1] = trend_records(hist, S, H, n + 1)
    # non-vacuity, on the oracle's output of the last step, before the GPU is asked
    rec = want[steps]
    usable, mk = rec[..., 3].astype(np.int64), rec[..., 2].view(np.int32)
    assert (usable < H).any() and (usable < 2).any() and (usable == H).any()
    free = n_ranks * (2 + 2 * S) - (n_ranks if S >= 1 else 1)
    assert free < 8 or ((mk > 0).any() and (mk < 0).any())
    assert plants == 0 or (mk < 0).any()
    near = _tied_or_adjacent(hist, S, H, steps)
    assert near.mean() >= 0.25, near.mean()
    assert any((w[..., 3] < min(k, H)).any() for k, w in want.items() if k <= H)  # while the ring fills, too
    return x, want, hist


@pytest.fixture(scope="module")
def lib():
    import torch

    from nvrx_straggler import _native

    assert torch.cuda.is_available()
    return _native.load()


@pytest.mark.parametrize("H,S,n_ranks", CASES, ids=[f"H{h}-S{s}-n{n}" for h, s, n in CASES])
def test_the_kernel_equals_the_restatement_bit_for_bit_and_only_reads_the_ring(lib, H, S, n_ranks):
    import torch

    from nvrx_straggler import _native

    x, want, hist = _expected(H, S, n_ranks)
    S_cap, R, steps = S + EXTRA_CAP, x.shape[1], x.shape[0]
    d_x = torch.from_numpy(x).cuda()
    d_hist = torch.full((_native.history_floats(n_ranks, S_cap, H) * 4,), 0xFF, dtype=torch.uint8, device="cuda")
    d_rec = torch.zeros(_native.history_words(n_ranks, S), dtype=torch.int32, device="cuda")
    words = _native.trend_words(n_ranks, S)
    d_out = torch.zeros(words + GUARD, dtype=torch.int32, device="cuda")
    thr = (ctypes.c_double * 4)(*THRESHOLDS)
    stream = torch.cuda.current_stream().cuda_stream
    for n in range(steps):
        rc = lib.nvrx_score_history(d_x[n].data_ptr(), R, S, FIRST_RANK, n_ranks, d_hist.data_ptr(), S_cap, H, n, thr,
                                    d_rec.data_ptr(), stream)
        assert rc == 0, lib.nvrx_last_error()
        if n + 1 not in want:
            continue
        before = d_hist.clone()
        d_out.fill_(-1)
        rc = lib.nvrx_score_trend(d_hist.data_ptr(), n_ranks, S, S_cap, H, n + 1, d_out.data_ptr(), stream)
        assert rc == 0, lib.nvrx_last_error()
        host = d_out.cpu().numpy().view(np.uint32)
        assert torch.equal(d_hist, before), n  # the kernel only reads the ring
        assert (host[words:] == 0xFFFFFFFF).all(), n  # nothing behind the records was written
        got = host[:words].reshape(n_ranks, 2, 1 + S, 4)
        if not np.array_equal(got, want[n + 1]):
            bad = np.argwhere((got != want[n + 1]).any(-1))[0]
            raise AssertionError((n, tuple(bad), got[tuple(bad)].tolist(), want[n + 1][tuple(bad)].tolist()))
    ring = d_hist.cpu().numpy().view(np.uint32).reshape(hist.shape)
    assert np.array_equal(ring, hist.view(np.uint32))  # (the ring the restatement was computed on)


def test_entries_beyond_f32s_range_apart_follow_the_contract(lib):
    """Pair slopes that overflow to +-inf, and the NaN v_a they make: canonical, ordered behind +inf."""
    import torch

    from nvrx_straggler import _native

    H, S, n = 8, 1, 1
    big = np.float32(3.0e38)
    nan = np.float32(np.nan)
    columns = ([nan, nan, nan, nan, -big, big],   # oldest first: the one pair slope is (big + big) / 1 = +inf, v_0 = inf * 0
               [nan, nan, nan, nan, big, -big],   # -inf
               [nan, nan, nan, big, -big, big],   # +inf, 0 and -inf: the median is the finite one
               [big, 1.0, -big, 2.0, big, 3.0])
    hist = fresh(n, S, H)
    for step in range(6):
        scores = np.array([[c[step] for c in columns]], dtype=np.float32)
        history_step(hist, scores, S, 0, n, H, step)
    want = trend_records(hist, S, H, 6)
    slopes, levels = want[..., 0].view(np.float32), want[..., 1].view(np.float32)
    assert sorted(slopes[np.isinf(slopes)].tolist()) == [-np.inf, np.inf] and np.isinf(levels).sum() == 2  # it is what it says
    d_hist = torch.from_numpy(hist.copy()).cuda()
    d_out = torch.zeros(_native.trend_words(n, S), dtype=torch.int32, device="cuda")
    rc = lib.nvrx_score_trend(d_hist.data_ptr(), n, S, S, H, 6, d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.nvrx_last_error()
    got = d_out.cpu().numpy().view(np.uint32).reshape(want.shape)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())


# ---- through the engine ---------------------------------------------------------------------------------------------------------
WINDOWS, LOCAL_RANKS, RING_CAP, ROWS = 12, 2, 64, ("falls", "flat", "once")
ONCE_WINDOW = 5
OPTIONS = dict(score_history=8, persistence_min_reports=3, score_trends=True, trend_min_reports=4, trend_min_tau=0.6)


def _fill(rings, rows, window):
    """Rank 0 is flat.  Rank 1's ``falls`` row is 3 % of the first window's pace slower every window (its relative score is
    1 / (1 + 0.03 w): 0.752 at the last window), its ``once`` row 1.5 x slower in one window only.  Integers: every sum is
    exact."""
    flat = np.full(RING_CAP, 1000.0, dtype=np.float32)
    for name in ROWS:
        rings.push_many(rows[name], flat, lr=0)
    rings.push_many(rows["falls"], np.full(RING_CAP, 1000.0 + 30.0 * window, dtype=np.float32), lr=1)
    rings.push_many(rows["flat"], flat, lr=1)
    rings.push_many(rows["once"], flat * np.float32(1.5 if window == ONCE_WINDOW else 1.0), lr=1)


def _run(be, asynchronous, **options):
    """``WINDOWS`` reports, unread until all were issued: per report its path, trends, declining stragglers and raw records."""
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=True, node_name="n",
                          asynchronous=asynchronous, **options)
    rings = be.make_rings(LOCAL_RANKS, len(ROWS), RING_CAP)
    rows = {name: rings.row_for(0, name) for name in ROWS}
    reports, planned = [], []
    try:
        for w in range(WINDOWS):
            _fill(rings, rows, w)
            planned.append(gen._ring_plan is not None)
            reports.append(gen.generate_report_from_rings(rings, rows, {}, local_ranks=LOCAL_RANKS))
            rings.reset()
        out = []
        for rep, was_planned in zip(reports, planned):
            src = rep.__dict__.get("_trends")
            out.append({"planned": was_planned, "records": None if src is None else np.array(src.handle.records()),
                        "trends": rep.score_trends(), "declining": rep.identify_declining_stragglers(),
                        "history": rep.score_history(), "stragglers": rep.identify_stragglers()})
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

    before, cpu = backend._backend, TrendOracleBackend()
    backend.set_backend(cpu)
    try:
        return _run(cpu, False, **OPTIONS)[0]
    finally:
        backend.set_backend(before)


def _same(a, b):
    import row_family_script as script

    return script.same(a, b)


@pytest.mark.parametrize("asynchronous", [False, True], ids=["synchronous", "asynchronous"])
def test_the_engine_gives_the_oracles_trends_on_the_general_and_the_planned_path(oracle_runs, asynchronous):
    from nvrx_straggler.backend import get_backend

    got, _ = _run(get_backend(), asynchronous, **OPTIONS)
    assert [e["planned"] for e in got] == [False] + [True] * (WINDOWS - 1)  # the general path once, then the cached plan
    named = []
    for w, (g, o) in enumerate(zip(got, oracle_runs)):
        assert np.array_equal(g["records"], o["records"]), w
        assert _same(g["trends"], o["trends"]), (w, g["trends"], o["trends"])
        assert g["declining"] == o["declining"] and g["stragglers"] == o["stragglers"] and _same(g["history"], o["history"]), w
        assert g["trends"]["depth"] == min(w + 1, 8) and g["trends"]["horizon"] == 8
        falls = g["trends"]["section_relative"]["falls"][1]
        assert falls["usable"] == min(w + 1, 8) and falls["falling"] == (w >= 3) and falls["tau"] == (-1.0 if w else 0.0)
        assert not g["trends"]["section_relative"]["once"][1]["falling"]
        assert (g["trends"]["section_relative"]["flat"][1]["slope"] == 0.0) == (w >= 1)
        named.append(sorted(s.rank for s in g["declining"]["straggler_sections_relative"].get("falls", ())))
        assert "once" not in g["declining"]["straggler_sections_relative"]
        assert not g["stragglers"]["straggler_sections_relative"].get("falls")  # no existing rule names it, to the end
    assert named[-1] == [1] and [] in named  # named ahead of its crossing, not from the start


@pytest.mark.parametrize("asynchronous", [False, True], ids=["synchronous", "asynchronous"])
def test_with_the_option_off_a_report_makes_no_trend_call(asynchronous):
    from nvrx_straggler.backend import get_backend

    be = get_backend()
    calls = []
    saved = {name: getattr(be, name) for name in ("score_trend", "trend_copy_out")}
    saved_lib = {name: getattr(be.lib, name) for name in ("nvrx_score_trend", "nvrx_report_trend")}

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
        history_only = dict(score_history=8, persistence_min_reports=3)
        off, gen = _run(be, asynchronous, **history_only)
        assert calls == [] and gen.score_trends is False
        assert all(e["trends"] == {} and e["records"] is None for e in off)
        ws = gen._ring_plan.ws if gen._ring_plan is not None else None
        assert ws is None or ws._trend_last is None
        plain, _ = _run(be, asynchronous)
        assert calls == [] and all(e["trends"] == {} for e in plain)
        on, _ = _run(be, asynchronous, **OPTIONS)
        steps = [c for c in calls if c.startswith("nvrx_")]
        assert len(steps) == WINDOWS and calls.count("trend_copy_out") == WINDOWS  # one launch and one copy-out per report
        for a, b in zip(off, on):  # ... and what a report says besides is the same either way
            assert a["stragglers"] == b["stragglers"] and _same(a["history"], b["history"])
    finally:
        for name, inner in saved.items():
            setattr(be, name, inner)
        for name, inner in saved_lib.items():
            setattr(be.lib, name, inner)
    # the CPU checker whose trend methods only count and raise: with the history on, the paths never reach for the trends
    from nvrx_straggler import backend

    before, counting = backend._backend, CountingTrendBackend(emulate_fused=True)
    backend.set_backend(counting)
    try:
        _run(counting, asynchronous, **history_only)
        assert counting.trend_calls == 0 and counting.history_calls == WINDOWS
    finally:
        backend.set_backend(before)
