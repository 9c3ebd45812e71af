"""Worker functions and input builders of the episode-score tests (importable by spawned processes).  The CPU workers install
the checker backend WITH episodes themselves, as their first statement (``mp_util.run_ranks`` installs the plain one)."""
import json
import pickle

import numpy as np

from tail_workers import record_collectives

RANKS, SECTIONS, SAMPLES = 8, 4, 2000
EPISODE_RANK, BURST_RANK, BEGIN, END = 3, 5, 1200, 1260  # 1.5 x on samples 1200 .. 1259: ended 740 samples ago
JOB_BEGIN, JOB_END = 700, 780
LEN_PPM = 5000  # the default episode_min_length


def _install_cpu_backend(**kw):
    from episode_oracle_backend import EpisodeOracleBackend
    from nvrx_straggler import backend

    be = EpisodeOracleBackend(**kw)
    backend.set_backend(be)
    return be


def headline_data():
    """8 ranks x 4 sections x 2000 samples around 1000 with 1 % noise; rank 3 is 1.5 x slower on samples 1200 .. 1259 (3 % of
    the window), rank 5 on a random 2 % of its samples."""
    rng = np.random.default_rng(17)
    base = (1000.0 * (1.0 + 0.01 * rng.standard_normal((RANKS, SECTIONS, SAMPLES)))).astype(np.float32)
    base[EPISODE_RANK, :, BEGIN:END] *= np.float32(1.5)
    bursts = rng.random((SECTIONS, SAMPLES)) < 0.02
    base[BURST_RANK] = np.where(bursts, base[BURST_RANK] * np.float32(1.5), base[BURST_RANK])
    return base


def jobwide_data():
    """The same job where EVERY rank is slow on samples 700 .. 779 (a checkpoint every rank takes)."""
    rng = np.random.default_rng(17)
    base = (1000.0 * (1.0 + 0.01 * rng.standard_normal((RANKS, SECTIONS, SAMPLES)))).astype(np.float32)
    base[:, :, JOB_BEGIN:JOB_END] *= np.float32(1.5)
    return base


def readme_row(slow=True):
    """The README's example: 10 000 samples around 1000 with 1 % noise, 1.5 x slower on samples 6000 .. 6299."""
    rng = np.random.default_rng(17)
    x = 1000.0 * (1.0 + 0.01 * rng.standard_normal(10000))
    if slow:
        x[6000:6300] *= 1.5
    return x.astype(np.float32)


def summarise(rep):
    """What the headline checks look at, as plain data."""
    found = rep.identify_stragglers()
    onset_found = rep.identify_onset_stragglers()
    period_found = rep.identify_period_stragglers()
    episode_found = rep.identify_episode_stragglers()
    return {
        "episodes": rep.episode_scores(),
        "periods": rep.period_scores(),
        "onsets": rep.onset_scores(),
        "tails": rep.tail_scores(),
        "section_relative": {n: dict(v) for n, v in rep.section_relative_perf_scores.items()},
        "median_flagged": sorted(s.rank for s in found["straggler_gpus_relative"])
        + sorted(s.rank for v in found["straggler_sections_relative"].values() for s in v),
        "onset_flagged": sorted(s.rank for s in onset_found["straggler_gpus_relative"])
        + sorted(s.rank for v in onset_found["straggler_sections_relative"].values() for s in v),
        "period_flagged": sorted(s.rank for s in period_found["straggler_gpus_relative"])
        + sorted(s.rank for v in period_found["straggler_sections_relative"].values() for s in v),
        "episode_sections": {n: sorted(s.rank for s in v) for n, v in episode_found["straggler_sections_relative"].items()},
        "episode_gpus": sorted(s.rank for s in episode_found["straggler_gpus_relative"]),
    }


def ring_reports_recorded(rank, world, gather_on_rank0, emulate_fused=False, asynchronous=False, tail_quantile=0.0,
                          onset_detection=False, period_detection=False):
    """Six ring reports on the checker backend; rank 1's section s0 is 1.5 x slower on samples 8 .. 15 of every window; a new
    section appears on the last rank at report 3 (the planned report falls back on every rank) and a new kernel on rank 0 at
    report 5.  Returns the collectives this rank issued, per report what was pushed, and what the report said."""
    be = _install_cpu_backend(emulate_fused=emulate_fused)
    calls = record_collectives()
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=gather_on_rank0,
                          node_name=f"node{rank}", episode_detection=True, asynchronous=asynchronous, tail_quantile=tail_quantile,
                          onset_detection=onset_detection, period_detection=period_detection)
    rings = be.make_rings(1, 16, 64)
    rng = np.random.default_rng(300 + rank)
    section_rows = {n: rings.row_for(0, n) for n in ("s0", "s1")}
    kernel_rows = {n: rings.row_for(1, n) for n in ("k0", "ncclDevKernel_z")}
    out, marks = [], []
    try:
        for i in range(6):
            if i == 2 and rank == world - 1:
                section_rows = dict(section_rows, s_new=rings.row_for(0, "s_new"))
            if i == 4 and rank == 0:
                kernel_rows = dict(kernel_rows, k_new=rings.row_for(1, "k_new"))
            pushed = {}
            for kind, table in (("section", section_rows), ("kernel", kernel_rows)):
                for name, row in table.items():
                    n = 6 + 9 * i + rank  # (6..53: the first two windows are too short for any episode)
                    v = (10.0 * (1.0 + 0.01 * rng.standard_normal(n))).astype(np.float32)
                    if rank == 1 and name == "s0":
                        v[8:16] *= np.float32(1.5)
                    rings.push_many(row, v)
                    pushed[f"{kind}:{name}"] = v.tolist()
            start = len(calls)
            rep = gen.generate_report_from_rings(rings, section_rows, kernel_rows)
            rings.reset()
            marks.append(calls[start:])
            entry = {"pushed": pushed, "episodes": None}
            if rep is not None:
                t = rep.episode_scores()
                json.dumps(t)
                entry["episodes"] = t
                entry["tails"] = rep.tail_scores()
                entry["onsets"] = rep.onset_scores()
                entry["periods"] = rep.period_scores()
                entry["flagged"] = {n: sorted(s.rank for s in v)
                                    for n, v in rep.identify_episode_stragglers()["straggler_sections_relative"].items()}
                entry["pickled_same"] = json.dumps(pickle.loads(pickle.dumps(rep)).episode_scores()) == json.dumps(t)
            out.append(entry)
        return {"calls": marks, "reports": out, "episode_local_calls": be.episode_local_calls,
                "episode_score_calls": be.episode_score_calls, "onset_enable_calls": be.onset_enable_calls,
                "onset_local_calls": be.onset_local_calls, "period_local_calls": be.period_local_calls}
    finally:
        gen.close()


# ---- inputs of the row-kernel tests (tests/test_gpu_episode.py; tests/test_episode_host.py checks them against the cap) ------
STRETCHES = ("at_5", "at_50", "at_90", "from_m", "to_n_minus_m", "middle")
KINDS = ("noise",) + STRETCHES + ("step", "ramp", "faster", "constant", "one_nan", "one_inf", "two_equal", "int_noise")
EXACT_KINDS = STRETCHES + ("two_equal", "int_noise", "constant")  # (a, b) is the oracle's, unconditionally
STRIDES = (4, 8, 24, 64, 256, 1000, 1024, 4096, 4100, 5000, 10000, 65536)
COUNTS = (0, 1, 23, 24, 25, 255, 256, 257)
PPMS = (1, 5000, 333333)
ROTATION_STRIDES = (64, 1000, 4100, 65536)
LAUNCHES = [(rows, stride) for stride in (64, 10000) for rows in (1, 2, 63, 512)]


def min_len(len_ppm, n):
    return max(8, (int(len_ppm) * int(n) + 999999) // 1000000)


def stretch_of(kind, n, m):
    """``(s, L)`` of the planted stretch [s, s + L) of a row of ``n`` samples: at least m long, at least m from either end
    where the row has room for that (n >= 3m); None where it has not."""
    if n < 3 * m:
        return None
    L = min(max(m, n // 20), n - 2 * m)
    s = {"at_5": n // 20, "at_50": n // 2, "at_90": (n * 9) // 10, "from_m": m, "to_n_minus_m": n - m - L,
         "middle": n // 2 - L // 2, "faster": n // 3}[kind]
    return min(max(s, m), n - m - L), L


def data_row(kind, rng, n, m):
    """One row of ``n`` >= 1 samples of the given kind (1 % noise around 1000 unless the kind says otherwise)."""
    x = 1000.0 * (1.0 + 0.01 * rng.standard_normal(n))
    if kind in STRETCHES or kind == "faster":
        where = stretch_of(kind, n, m)
        if where:
            s, L = where
            x[s : s + L] *= 0.5 if kind == "faster" else 1.5
    elif kind == "step":
        x[int(n * 0.7):] *= 1.5
    elif kind == "ramp":
        x += np.arange(n) * (300.0 / n)
    elif kind == "constant":
        x[:] = 1234.5
    elif kind == "one_nan":
        x[n // 2] = np.nan
    elif kind == "one_inf":
        x[n // 3] = np.inf
    elif kind == "two_equal":
        # two stretches of the same integer height and length on a flat integer baseline: their E is the same number, bit for
        # bit (every sum is exact), and the gap between them is long enough that the interval spanning both explains less
        x[:] = 1000.0
        L = max(m, n // 32)
        s1 = m + n // 16
        s2 = s1 + L + (n * 5) // 8
        if s2 + L <= n - m:
            x[s1 : s1 + L] = 1500.0
            x[s2 : s2 + L] = 1500.0
        else:  # (no room for two: one)
            where = stretch_of("middle", n, m)
            if where:
                x[where[0] : where[0] + where[1]] = 1500.0
    elif kind == "int_noise":
        x = rng.integers(990, 1011, n).astype(np.float64)
    return x.astype(np.float32)


def two_equal_first(n, m):
    """``(a, b)`` of the FIRST of the two equal stretches of a ``two_equal`` row, None where only one was planted."""
    L = max(m, n // 32)
    s1 = m + n // 16
    s2 = s1 + L + (n * 5) // 8
    return (s1, s1 + L) if s2 + L <= n - m else None


def _pad(x, stride):
    row = np.zeros(stride, dtype=np.float32)
    row[: x.size] = x
    return row


def kernel_case(stride, len_ppm):
    """``(samples [rows, stride], counts, kinds [rows])`` of one stride and minimum length: every kind at counts 0, 1, 23, 24,
    25, 255, 256, 257 and the full stride (clamped to the stride).  Samples behind a row's count are filled with a value no
    sum may pick up."""
    rng = np.random.default_rng(7000 + stride * 7 + len_ppm % 1000)
    rows, counts, kinds = [], [], []
    for kind in KINDS:
        for n in sorted({min(c, stride) for c in COUNTS + (stride,)}):
            x = data_row(kind, rng, n, min_len(len_ppm, n)) if n else np.zeros(0, dtype=np.float32)
            row = np.full(stride, 3.0e30, dtype=np.float32)
            row[: x.size] = x
            rows.append(row)
            counts.append(n)
            kinds.append(kind)
    return np.stack(rows), np.array(counts, dtype=np.uint32), kinds


def rotation_case(stride, len_ppm=LEN_PPM):
    """Full rows, each at ring starts 0, 1, 3, n/2 and n-1 (five consecutive rows hold the same samples in time order)."""
    rng = np.random.default_rng(8000 + stride)
    rows, starts, kinds = [], [], []
    m = min_len(len_ppm, stride)
    for kind in KINDS:
        x = data_row(kind, rng, stride, m)
        for start in (0, 1, 3, stride // 2, stride - 1):
            rows.append(np.roll(x, start))
            starts.append(start)
            kinds.append(kind)
    return np.stack(rows), np.full(len(rows), stride, dtype=np.uint32), np.array(starts, dtype=np.uint32), kinds


def launch_case(rows, stride, len_ppm=LEN_PPM):
    """Many rows in one launch: every kind in turn, some rows short."""
    rng = np.random.default_rng(9000 + rows + stride)
    counts = np.full(rows, stride, dtype=np.uint32)
    counts[5::11] = rng.integers(0, stride + 1, counts[5::11].size)
    samples, kinds = [], []
    for r in range(rows):
        kind = KINDS[r % len(KINDS)]
        n = int(counts[r])
        x = data_row(kind, rng, n, min_len(len_ppm, n)) if n else np.zeros(0, dtype=np.float32)
        samples.append(_pad(x, stride))
        kinds.append(kind)
    return np.stack(samples), counts, kinds


def band_tol(ep):
    """The width of the undecided band of a row, in units of E: 1e-10 * A, A = sum |d_i| (tests/test_gpu_episode.py argues
    it)."""
    return 1e-10 * ep.A


def in_band(ep):
    """Whether the bounds do not pin down the interval of this row: another b's best E lies within the band of the largest,
    the largest within the band of 0, or -- for the winning b -- the second-smallest admissible H_a within the band of the
    smallest."""
    if ep is None or ep.M is None:
        return False
    tol = band_tol(ep)
    M = ep.M
    k = int(np.argmax(M))
    top = float(M[k])
    if abs(top) <= tol:
        return True
    if not top > 0.0:
        return False
    others = np.delete(M, k)
    if others.size and float(others.max()) >= top - tol:
        return True
    b = 2 * ep.m + k
    H = np.sort(ep.H[ep.m : b - ep.m + 1])
    return H.size > 1 and float(H[1] - H[0]) / ep.n <= tol


def band_rows(eps, kinds):
    """Rows inside the undecided band, among those whose interval is not promised unconditionally."""
    return [r for r, ep in enumerate(eps) if kinds[r] not in EXACT_KINDS and in_band(ep)]


# ---- GPU workers (product backend) -------------------------------------------------------------------------------------
def folded_headline(rank, world, tail_quantile=0.0, onset_detection=False, period_detection=False):
    """The headline shape through FoldedJob on the product backend, ``world`` processes sharing the GPU."""
    from nvrx_straggler.folded import FoldedJob

    data = headline_data()
    calls = record_collectives()
    job = FoldedJob(total_ranks=RANKS, sections=SECTIONS, ring_cap=SAMPLES, scores_to_compute=("relative_perf_scores",),
                    node_name=f"node{rank}", episode_detection=True, tail_quantile=tail_quantile, onset_detection=onset_detection,
                    period_detection=period_detection)
    try:
        out = []
        for _ in range(3):  # the general report, then planned ones
            for lr, r in enumerate(job.logical_ranks()):
                job.load(lr, data[r])
            start = len(calls)
            rep = job.report()
            rows = [c[1] for c in calls[start:] if c[0] == "rows"]
            out.append({"rows": rows, "report": None if rep is None else summarise(rep)})
        return out
    finally:
        job.close()


def planted_window_row(rng, n, m):
    """1 % noise and one 1.5 x stretch of a length and place of the row's own."""
    x = 1000.0 * (1.0 + 0.01 * rng.standard_normal(n))
    L = int(rng.integers(max(m, n // 50), n // 8))
    s = int(rng.integers(m, n - m - L))
    x[s : s + L] *= 1.5
    return x.astype(np.float32), s, L


def ring_windows_written_from_another_stream(rank, world, asynchronous, windows=12):
    """Device rings + ReportGenerator.generate_report_from_rings in one process, one logical rank, 8 sections x 4096 samples,
    every row of every window with a planted stretch of its own.  Right after each report call returns, the NEXT window's
    samples -- ten times larger or smaller, their stretches elsewhere -- are appended with ``nvrx_ring_push_device`` from a
    stream of the test's own.  Returns every report's section episodes, the windows' samples, and how often the episodes' one
    copy-out had run."""
    import torch

    from nvrx_straggler import _native
    from nvrx_straggler.backend import get_backend
    from nvrx_straggler.reporting import ReportGenerator

    torch.cuda.set_device(0)
    be = get_backend()
    S, n = 8, 4096
    rings = be.make_rings(1, S, n)
    gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=True, node_name="n", asynchronous=asynchronous,
                          episode_detection=True)
    names = [f"sec{s}" for s in range(S)]
    rows = {name: rings.row_for(_native.KIND_SECTION, name) for name in names}
    no_kernels = {}
    calls = [0]
    inner = be.episodes_copy_out

    def counted(t):
        calls[0] += 1
        return inner(t)

    be.episodes_copy_out = counted
    rng = np.random.default_rng(12)
    m = min_len(LEN_PPM, n)
    host = np.zeros((windows, S, n), dtype=np.float32)
    planted = np.zeros((windows, S, 2), dtype=np.int64)
    for w in range(windows):
        for s in range(S):
            x, at, L = planted_window_row(rng, n, m)
            host[w, s] = x * np.float32(0.1)
            planted[w, s] = (at, L)
    host[1::2] *= np.float32(10.0)
    dev = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    other = torch.cuda.Stream()

    def push(w):
        for s, name in enumerate(names):
            _native.check(be.lib.nvrx_ring_push_device(rings.ctx, rows[name], dev[w, s].data_ptr(), n, other.cuda_stream))

    try:
        out = []
        push(0)
        other.synchronize()  # (the report reads what is in the rings: the first window has landed)
        for w in range(windows):
            rep = gen.generate_report_from_rings(rings, rows, no_kernels)
            rings.reset()
            if w + 1 < windows:
                push(w + 1)  # at once, from another stream, over the slots the report's kernels read
            at_return = calls[0]
            rep.identify_stragglers()
            dict(rep.section_relative_perf_scores)
            before = calls[0]
            t = rep.episode_scores()
            after_first = calls[0]
            rep.episode_scores()
            out.append({"section_episodes": {k: v[0] for k, v in t["section_episodes"].items()},
                        "section_relative": {k: v[0] for k, v in t["section_relative"].items()},
                        "copy_outs": (at_return, before, after_first, calls[0])})
            other.synchronize()  # the next report reads the next window
        return {"reports": out, "samples": host, "names": names, "planted": planted}
    finally:
        gen.close()
        rings.close()


def wrapped_ring(rank, world, ring_cap=64):
    """One and a half ring capacities of samples (and two and five more) pushed into 64-deep rings, between windows that do
    not wrap; every section with a stretch of its own near the end of what was pushed.  Returns the episodes and what was
    pushed."""
    import torch

    from nvrx_straggler import _native
    from nvrx_straggler.backend import get_backend
    from nvrx_straggler.reporting import ReportGenerator

    torch.cuda.set_device(0)
    be = get_backend()
    rings = be.make_rings(1, 4, ring_cap)
    gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=True, node_name="n", episode_detection=True)
    names = [f"sec{s}" for s in range(4)]
    rows = {name: rings.row_for(_native.KIND_SECTION, name) for name in names}
    rng = np.random.default_rng(13)
    try:
        out = []
        for pushes in (ring_cap * 3 // 2, ring_cap, ring_cap * 2 + 5, ring_cap - 9):
            pushed = (10.0 * (1.0 + 0.01 * rng.standard_normal((4, pushes)))).astype(np.float32)
            for s in range(4):  # 8 + s slow samples that end 10 + 3 s samples before the last one pushed
                end = pushes - 10 - 3 * s
                pushed[s, end - 8 - s : end] *= np.float32(1.5)
            for s, name in enumerate(names):
                rings.push_many(rows[name], pushed[s])
            rep = gen.generate_report_from_rings(rings, rows, {})
            rings.reset()
            out.append({"episodes": rep.episode_scores()["section_episodes"], "pushed": pushed})
        return {"windows": out, "names": names}
    finally:
        gen.close()
        rings.close()
