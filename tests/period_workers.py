"""Worker functions and input builders of the period-score tests (importable by spawned processes).  The CPU workers install
the checker backend WITH periods themselves, as their first statement (``mp_util.run_ranks`` installs the plain one)."""
import json
import pickle

import numpy as np

from tail_workers import record_collectives

RANKS, SECTIONS, SAMPLES = 8, 4, 2000
BEAT_RANK, BURST_RANK, BEAT, BEAT_PHASE = 3, 5, 50, 13  # 1.5 x on samples 13, 63, ...: last seen (1999 - 13) % 50 = 36 ago
JOB_BEAT, JOB_PHASE = 100, 7


def _install_cpu_backend(**kw):
    from nvrx_straggler import backend
    from period_oracle_backend import PeriodOracleBackend

    be = PeriodOracleBackend(**kw)
    backend.set_backend(be)
    return be


def headline_data():
    """8 ranks x 4 sections x 2000 samples around 1000 with 1 % noise; rank 3 is 1.5 x slower on every 50th sample, rank 5
    on a random 2 % of its samples (the same share, without a beat)."""
    rng = np.random.default_rng(17)
    base = (1000.0 * (1.0 + 0.01 * rng.standard_normal((RANKS, SECTIONS, SAMPLES)))).astype(np.float32)
    base[BEAT_RANK, :, BEAT_PHASE::BEAT] *= np.float32(1.5)
    bursts = rng.random((SECTIONS, SAMPLES)) < 0.02
    base[BURST_RANK] = np.where(bursts, base[BURST_RANK] * np.float32(1.5), base[BURST_RANK])
    return base


def jobwide_data():
    """The same job where EVERY rank stalls on every 100th sample (an eval, a checkpoint every rank takes)."""
    rng = np.random.default_rng(17)
    base = (1000.0 * (1.0 + 0.01 * rng.standard_normal((RANKS, SECTIONS, SAMPLES)))).astype(np.float32)
    base[:, :, JOB_PHASE::JOB_BEAT] *= np.float32(1.5)
    return base


def summarise(rep):
    """What the headline checks look at, as plain data."""
    found = rep.identify_stragglers()
    onset_found = rep.identify_onset_stragglers()
    period_found = rep.identify_period_stragglers()
    return {
        "periods": rep.period_scores(),
        "onsets": rep.onset_scores(),
        "tails": rep.tail_scores(),
        "section_relative": {n: dict(v) for n, v in rep.section_relative_perf_scores.items()},
        "median_flagged": sorted(s.rank for s in found["straggler_gpus_relative"])
        + sorted(s.rank for v in found["straggler_sections_relative"].values() for s in v),
        "onset_flagged": sorted(s.rank for s in onset_found["straggler_gpus_relative"])
        + sorted(s.rank for v in onset_found["straggler_sections_relative"].values() for s in v),
        "period_sections": {n: sorted(s.rank for s in v) for n, v in period_found["straggler_sections_relative"].items()},
        "period_gpus": sorted(s.rank for s in period_found["straggler_gpus_relative"]),
    }


def ring_reports_recorded(rank, world, gather_on_rank0, emulate_fused=False, asynchronous=False, tail_quantile=0.0,
                          onset_detection=False):
    """Six ring reports on the checker backend; rank 1's section s0 stalls on every 3rd sample of every window; a new section
    appears on the last rank at report 3 (the planned report falls back on every rank) and a new kernel on rank 0 at report
    5.  Returns the collectives this rank issued, per report what was pushed, and what the report said."""
    be = _install_cpu_backend(emulate_fused=emulate_fused)
    calls = record_collectives()
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=gather_on_rank0,
                          node_name=f"node{rank}", period_detection=True, asynchronous=asynchronous, tail_quantile=tail_quantile,
                          onset_detection=onset_detection)
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
                    n = 6 + 9 * i + rank  # (6..53: the first window is too short for any period)
                    v = (10.0 * (1.0 + 0.01 * rng.standard_normal(n))).astype(np.float32)
                    if rank == 1 and name == "s0":
                        v[1::3] *= np.float32(1.5)
                    rings.push_many(row, v)
                    pushed[f"{kind}:{name}"] = v.tolist()
            start = len(calls)
            rep = gen.generate_report_from_rings(rings, section_rows, kernel_rows)
            rings.reset()
            marks.append(calls[start:])
            entry = {"pushed": pushed, "periods": None}
            if rep is not None:
                t = rep.period_scores()
                json.dumps(t)
                entry["periods"] = t
                entry["tails"] = rep.tail_scores()
                entry["onsets"] = rep.onset_scores()
                entry["flagged"] = {n: sorted(s.rank for s in v)
                                    for n, v in rep.identify_period_stragglers()["straggler_sections_relative"].items()}
                entry["pickled_same"] = json.dumps(pickle.loads(pickle.dumps(rep)).period_scores()) == json.dumps(t)
            out.append(entry)
        return {"calls": marks, "reports": out, "period_local_calls": be.period_local_calls,
                "period_score_calls": be.period_score_calls, "onset_enable_calls": be.onset_enable_calls,
                "onset_local_calls": be.onset_local_calls}
    finally:
        gen.close()


# ---- inputs of the row-kernel tests (tests/test_gpu_period.py; tests/test_period_host.py checks them against the cap) --------
NO_BEAT = ("noise", "step", "ramp", "bursts", "constant", "one_nan", "one_inf")
PLANTED = (2, 7, 63, 64, 65, 128, 129)
LDS_SAMPLES = 10240  # rows up to this many samples are staged in LDS ("Period scores")
STRIDES = (8, 64, 256, 1000, 4096, 4100, LDS_SAMPLES, LDS_SAMPLES + 4, 65536)


def max_period_for(stride):
    return 1024 if stride <= 4096 else (64 if stride == 65536 else 128)


def plain_row(kind, rng, n):
    """One row of ``n`` samples around 1000 with 1 % noise and no beat."""
    x = 1000.0 * (1.0 + 0.01 * rng.standard_normal(n))
    if kind == "step":
        x[int(n * 0.7):] *= 1.5
    elif kind == "ramp":
        x += np.arange(n) * (300.0 / max(n, 1))
    elif kind == "bursts":
        x = np.where(rng.random(n) < 0.10, x * 1.5, x)
    elif kind == "constant":
        x[:] = 1234.5
    elif kind == "one_nan":
        x[n // 2] = np.nan
    elif kind == "one_inf":
        x[n // 3] = np.inf
    return x.astype(np.float32)


def planted_row(rng, n, P, width):
    """1 % noise and ``width`` consecutive 1.5 x samples in every ``P``, from a phase of the row's own."""
    x = 1000.0 * (1.0 + 0.01 * rng.standard_normal(n))
    first = int(rng.integers(0, P))
    slow = ((np.arange(n) - first) % P) < width
    x[slow] *= 1.5
    return x.astype(np.float32)


def kernel_case(stride):
    """``(samples [rows, stride], counts, max_period, planted [rows])`` of one stride: every row without a beat at counts 0,
    1, 7, 8, 9 and the full stride; every planted period that fits (and Pmax itself), one slow sample per period and five
    consecutive ones (five of two is a constant row: period 2 takes the single one only), at counts 4P - 1, 4P and the full
    stride.  ``planted[r]`` is the period the row must show, 0 where nothing is promised (no beat, or fewer than four
    repetitions)."""
    rng = np.random.default_rng(7000 + stride)
    max_period = max_period_for(stride)
    pmax = min(max_period, stride // 4)
    rows, counts, planted = [], [], []

    def add(x, n, P):
        row = np.zeros(stride, dtype=np.float32)
        row[: x.size] = x
        rows.append(row)
        counts.append(n)
        planted.append(P)

    for kind in NO_BEAT:
        for n in sorted({min(c, stride) for c in (0, 1, 7, 8, 9, stride)}):
            add(plain_row(kind, rng, stride), n, 0)
    for P in sorted({p for p in PLANTED + (pmax,) if 2 <= p <= pmax}):
        for width in (1, 5):
            if width > 1 and width >= P - 1:
                continue
            for n in sorted({c for c in (4 * P - 1, 4 * P, stride) if c <= stride}):
                add(planted_row(rng, stride, P, width), n, P if min(max_period, n // 4) >= P else 0)
    return np.stack(rows), np.array(counts, dtype=np.uint32), max_period, np.array(planted, dtype=np.int64)


def rotation_case(stride):
    """Full rows, each at ring starts 0, 1, 3, n/2 and n-1 (five consecutive rows hold the same samples in time order), the
    planted period no divisor of the row's length."""
    rng = np.random.default_rng(8000 + stride)
    max_period = max_period_for(stride)
    rows, starts, planted = [], [], []
    beats = [P for P in (7, 63, 65, 127) if P <= min(max_period, stride // 4) and stride % P]
    for x, P in [(plain_row(k, rng, stride), 0) for k in NO_BEAT] + [(planted_row(rng, stride, P, 1), P) for P in beats]:
        for start in (0, 1, 3, stride // 2, stride - 1):
            rows.append(np.roll(x, start))
            starts.append(start)
            planted.append(P)
    return (np.stack(rows), np.full(len(rows), stride, dtype=np.uint32), np.array(starts, dtype=np.uint32), max_period,
            np.array(planted, dtype=np.int64))


def launch_case(rows, stride):
    """Many rows in one launch: every kind in turn, planted rows among them, some rows short."""
    rng = np.random.default_rng(9000 + rows)
    max_period = max_period_for(stride)
    pmax = min(max_period, stride // 4)
    beats = [P for P in PLANTED if P <= pmax // 2]
    samples, planted = [], []
    for r in range(rows):
        k = r % (len(NO_BEAT) + 3)
        if k < len(NO_BEAT):
            samples.append(plain_row(NO_BEAT[k], rng, stride))
            planted.append(0)
        else:
            P = beats[(r // 10) % len(beats)]
            samples.append(planted_row(rng, stride, P, 1 if k % 2 or P < 7 else 5))
            planted.append(P)
    counts = np.full(rows, stride, dtype=np.uint32)
    counts[5::11] = rng.integers(0, stride + 1, counts[5::11].size)
    planted = np.array(planted, dtype=np.int64)
    planted[counts != stride] = 0  # (a short row promises nothing)
    return np.stack(samples), counts, max_period, planted


def band_rows(curves, tol=1e-9):
    """Rows whose choice of period the bounds do not pin down: some candidate lies within ``tol`` of the bar 0.95 * a_max, or
    a_max itself within ``tol`` of 0."""
    out = []
    for r, c in enumerate(curves):
        if c is None or c.size == 0:
            continue
        a_max = float(c.max())
        if abs(a_max) <= tol or (a_max > 0 and np.any(np.abs(c - 0.95 * a_max) <= tol)):
            out.append(r)
    return out


# ---- GPU workers (product backend) -------------------------------------------------------------------------------------
def folded_headline(rank, world, tail_quantile=0.0, onset_detection=False):
    """The headline shape through FoldedJob on the product backend, ``world`` processes sharing the GPU."""
    from nvrx_straggler.folded import FoldedJob

    data = headline_data()
    calls = record_collectives()
    job = FoldedJob(total_ranks=RANKS, sections=SECTIONS, ring_cap=SAMPLES, scores_to_compute=("relative_perf_scores",),
                    node_name=f"node{rank}", period_detection=True, tail_quantile=tail_quantile, onset_detection=onset_detection)
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


def ring_windows_written_from_another_stream(rank, world, asynchronous, windows=12):
    """Device rings + ReportGenerator.generate_report_from_rings in one process, one logical rank, 8 sections x 4096 samples,
    every row of every window with a planted period of its own.  Right after each report call returns, the NEXT window's
    samples -- ten times larger or smaller, on another beat -- are appended with ``nvrx_ring_push_device`` from a stream of
    the test's own.  Returns every report's section periods, the windows' samples, and how often the periods' one copy-out
    had run."""
    import torch

    from nvrx_straggler import _native
    from nvrx_straggler.backend import get_backend
    from nvrx_straggler.reporting import ReportGenerator

    torch.cuda.set_device(0)
    be = get_backend()
    S, n = 8, 4096
    rings = be.make_rings(1, S, n)
    gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=True, node_name="n", asynchronous=asynchronous,
                          period_detection=True, period_max=128)
    names = [f"sec{s}" for s in range(S)]
    rows = {name: rings.row_for(_native.KIND_SECTION, name) for name in names}
    no_kernels = {}
    calls = [0]
    inner = be.periods_copy_out

    def counted(t):
        calls[0] += 1
        return inner(t)

    be.periods_copy_out = counted
    rng = np.random.default_rng(12)
    beats = rng.integers(5, 100, (windows, S))
    host = np.stack([np.stack([planted_row(rng, n, int(beats[w, s]), 1) * np.float32(0.1) for s in range(S)])
                     for w in range(windows)]).astype(np.float32)
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
            t = rep.period_scores()
            after_first = calls[0]
            rep.period_scores()
            out.append({"section_periods": {k: v[0] for k, v in t["section_periods"].items()},
                        "section_relative": {k: v[0] for k, v in t["section_relative"].items()},
                        "copy_outs": (at_return, before, after_first, calls[0])})
            other.synchronize()  # the next report reads the next window
        return {"reports": out, "samples": host, "names": names, "beats": beats}
    finally:
        gen.close()
        rings.close()


def wrapped_ring(rank, world, ring_cap=64):
    """One and a half ring capacities of samples (and two and five more) pushed into 64-deep rings, between windows that do
    not wrap; every section on a beat of its own.  Returns the periods and what was pushed."""
    import torch

    from nvrx_straggler import _native
    from nvrx_straggler.backend import get_backend
    from nvrx_straggler.reporting import ReportGenerator

    torch.cuda.set_device(0)
    be = get_backend()
    rings = be.make_rings(1, 4, ring_cap)
    gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=True, node_name="n", period_detection=True)
    names = [f"sec{s}" for s in range(4)]
    rows = {name: rings.row_for(_native.KIND_SECTION, name) for name in names}
    rng = np.random.default_rng(13)
    try:
        out = []
        for pushes in (ring_cap * 3 // 2, ring_cap, ring_cap * 2 + 5, ring_cap - 9):
            pushed = np.stack([planted_row(rng, pushes, 4 + s, 1) * np.float32(0.01) for s in range(4)])  # periods 4, 5, 6, 7
            for s, name in enumerate(names):
                rings.push_many(rows[name], pushed[s])
            rep = gen.generate_report_from_rings(rings, rows, {})
            rings.reset()
            out.append({"periods": rep.period_scores()["section_periods"], "pushed": pushed})
        return {"windows": out, "names": names}
    finally:
        gen.close()
        rings.close()
