"""Worker functions and scenarios of the pace-score tests (importable by spawned processes).  The CPU workers install the
checker backend WITH pace scores themselves, as their first statement (``mp_util.run_ranks`` installs the plain one)."""
import pickle

import numpy as np

RANKS, KERNELS, SLOW_RANK, SAMPLES = 8, 120, 5, 200
SCENARIOS = ("slow_4pct", "nobody", "slow_1p5pct", "slow_4pct_bins", "slow_in_few")
NAMED = {"slow_4pct": [SLOW_RANK], "nobody": [], "slow_1p5pct": [], "slow_4pct_bins": [SLOW_RANK], "slow_in_few": []}


def scenario_medians(kind, ranks=RANKS, kernels=KERNELS, seed=2026):
    """``[ranks, kernels]`` f32 kernel medians in microseconds: lognormal kernel times (around 100 us, sigma 0.5: no single
    kernel carries the window), 1 % noise per entry, and
    ``slow_4pct``      rank 5 4 % slower in every kernel;
    ``nobody``         nobody is slow;
    ``slow_1p5pct``    rank 5 1.5 % slower in every kernel (below the rule's effect size);
    ``slow_4pct_bins`` rank 5 4 % slower, plus a fixed offset within +-1 % per rank ("silicon bins");
    ``slow_in_few``    rank 5 1.5 x slower in 5 % of its kernels (kernel attribution's case, not this one)."""
    assert kind in SCENARIOS
    rng = np.random.default_rng(seed)
    base = rng.lognormal(np.log(100.0), 0.5, kernels)
    med = base[None, :] * (1.0 + 0.01 * rng.standard_normal((ranks, kernels)))
    if kind in ("slow_4pct", "slow_4pct_bins"):
        med[SLOW_RANK] *= 1.04
    if kind == "slow_1p5pct":
        med[SLOW_RANK] *= 1.015
    if kind == "slow_4pct_bins":
        med *= (1.0 + rng.uniform(-0.01, 0.01, ranks))[:, None]
    if kind == "slow_in_few":
        med[SLOW_RANK, 10::20] *= 1.5  # (every 20th kernel)
    return med.astype(np.float32)


def ranks_named(found):
    """Ranks named anywhere in an ``identify_*stragglers`` result."""
    ranks = set()
    for v in found.values():
        for group in (v.values() if isinstance(v, dict) else [v]):
            ranks |= {s.rank for s in group}
    return sorted(ranks)


def _install_cpu_backend(**kw):
    from nvrx_straggler import backend
    from pace_oracle_backend import PaceOracleBackend

    be = PaceOracleBackend(**kw)
    backend.set_backend(be)
    return be


def ring_reports_recorded(rank, world, gather_on_rank0, pace=True, emulate_fused=False, asynchronous=False):
    """Six ring reports on the checker backend; a new section appears on the last rank at report 3 and a new kernel on rank 0
    at report 5.  Returns the collectives this rank issued per report and what the reports said."""
    from tail_workers import record_collectives

    be = _install_cpu_backend(emulate_fused=emulate_fused)
    calls = record_collectives()
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=gather_on_rank0,
                          node_name=f"node{rank}", pace_scores=pace, pace_min_ranks=2, asynchronous=asynchronous)
    rings = be.make_rings(1, 16, 64)
    rng = np.random.default_rng(100 + rank)
    section_rows = {n: rings.row_for(0, n) for n in ("s0", "s1")}
    kernel_rows = {n: rings.row_for(1, n) for n in ("k0", "k1", "ncclDevKernel_z")}
    out, marks = [], []
    try:
        for i in range(6):
            if i == 2 and rank == world - 1:
                section_rows = dict(section_rows, s_new=rings.row_for(0, "s_new"))
            if i == 4 and rank == 0:
                kernel_rows = dict(kernel_rows, k_new=rings.row_for(1, "k_new"))
            for table in (section_rows, kernel_rows):
                for row in table.values():
                    rings.push_many(row, rng.lognormal(2.0 + 0.1 * rank, 0.3, 11 + 3 * i + rank).astype(np.float32))
            start = len(calls)
            rep = gen.generate_report_from_rings(rings, section_rows, kernel_rows)
            rings.reset()
            marks.append(calls[start:])
            entry = {"pace": None}
            if rep is not None:
                t = rep.pace_scores()
                entry["pace"] = t
                entry["pickled_same"] = repr(pickle.loads(pickle.dumps(rep)).pace_scores()) == repr(t)
            out.append(entry)
        return {"calls": marks, "reports": out, "pace_calls": be.pace_calls, "pace_args": be.pace_args}
    finally:
        gen.close()


# ---- GPU workers (product backend) -------------------------------------------------------------------------------------
KERNEL_NAMES = tuple(f"kernel_{k:03d}" for k in range(KERNELS))


def folded_pace(rank, world, kind="slow_4pct", reports=3, asynchronous=False):
    """The scenario through FoldedJob on the product backend (one section, the step, next to the 120 kernel rows): the general
    report, then planned ones.  Per report: what it said, whom each rule names, the table it was computed from (read back
    from the workspace) and what ``backend.pace_score`` says of that same table."""
    import torch

    from nvrx_straggler.backend import get_backend
    from nvrx_straggler.folded import FoldedJob

    torch.cuda.set_device(0)
    med = scenario_medians(kind)
    job = FoldedJob(total_ranks=RANKS, section_names=["step"], ring_cap=256, scores_to_compute=("relative_perf_scores",),
                    node_name=f"node{rank}", kernel_names=KERNEL_NAMES, pace_scores=True, robust_scores=True,
                    asynchronous=asynchronous)
    be = get_backend()
    try:
        out = []
        for i in range(reports):
            for lr, r in enumerate(job.logical_ranks()):
                job.load(lr, np.full((1, SAMPLES), med[r].sum(), dtype=np.float32))
                job.load_kernels(lr, np.repeat(med[r][:, None], SAMPLES, axis=1))
            rep = job.report()
            entry = {"pace": rep.pace_scores(), "named": ranks_named(rep.identify_pace_stragglers()),
                     "job_named": ranks_named(rep.identify_stragglers()),
                     "robust_named": ranks_named(rep.identify_robust_stragglers()),
                     "fused": getattr(job.reporter, "_last_plan_fused", None),
                     "rehomed": int(job.rings.lib.nvrx_ctx_info(job.rings.ctx, 5))}
            plan = job.reporter._ring_plan
            if plan is not None:
                ws = plan.ws
                be.synchronize()
                torch.cuda.synchronize()
                entry["shape"] = (ws.R, ws.K, ws.S)
                entry["table"] = ws.table.cpu().numpy().copy()
                entry["direct"] = be.pace_score(ws, ws.table, 0, ws.R, min(4, ws.R)).records()
            out.append(entry)
        return out
    finally:
        job.close()


def folded_pace_sync_then_async(rank, world, **options):
    """``folded_pace`` twice in one process: synchronous reports, then asynchronous ones (each with rings of its own)."""
    return {"sync": folded_pace(rank, world, asynchronous=False, **options),
            "async": folded_pace(rank, world, asynchronous=True, **options)}


def held_reports(rank, world, windows=5):
    """Reports held across the next two on the same workspace: every window's kernel takes another time, and each report is
    read only after two more were issued."""
    import torch

    from nvrx_straggler.folded import FoldedJob

    torch.cuda.set_device(0)
    job = FoldedJob(total_ranks=4, section_names=["step"], ring_cap=64, scores_to_compute=("relative_perf_scores",),
                    kernel_names=("gemm",), pace_scores=True, pace_min_ranks=2)
    try:
        held, out = [], []
        for w in range(windows):
            for lr in range(4):
                job.load(lr, np.full((1, 9), 100.0 * (w + 1) + lr, dtype=np.float32))
                job.load_kernels(lr, np.full((1, 9), 10.0 * (w + 1) + lr, dtype=np.float32))
            held.append(job.report())
            if w >= 2:
                out.append(held[w - 2].pace_scores())
        out.extend(h.pace_scores() for h in held[-2:])
        return out
    finally:
        job.close()


def detector_rehomed(rank, world, windows=12, sections=3):
    """Asynchronous Detector reports with pace scores, re-homed onto the stream their stamps ran on (forced by a 1 us gap):
    section i of window t holds samples of 10 t + i only, so a pace step that read another window's table would show another
    center.  Per report: what it said, the table it was computed from (read back from the workspace once the window's work
    has run) and what ``backend.pace_score`` says of that same table."""
    import torch

    from nvrx_straggler import Detector
    from nvrx_straggler.backend import get_backend

    Detector.initialize(scores_to_compute="all", gather_on_rank0=True, node_name="n", asynchronous=True, pace_scores=True)
    try:
        names = [f"s{i}" for i in range(sections)]
        for name in names:
            with Detector.detection_section(name, profile_cuda=True):
                pass
        Detector.generate_report()
        rings, be = Detector.rings, get_backend()
        secs = [Detector.custom_sections[name] for name in names]
        gpu_rows = [rings.kernel_row_names[f"hipevent::{name}"] for name in names]
        big = torch.randn(4096, 4096, device="cuda")
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        torch.cuda.synchronize()
        out = []
        for t in range(1, windows + 1):
            st = streams[t % 2]
            with torch.cuda.stream(st):
                (big @ big).sum()  # the report of this window queues behind it on this stream
                for i, (sec, gpu_row) in enumerate(zip(secs, gpu_rows)):
                    for _ in range(3):
                        rings.stamp_begin(gpu_row, st.cuda_stream)
                        rings.stamp_end(gpu_row, st.cuda_stream, sec.row, float(10 * t + i))
                rep = Detector.generate_report()  # returns at once; re-homed onto `st`
            torch.cuda.synchronize()
            be.synchronize()
            entry = {"pace": rep.pace_scores()}
            plan = Detector.reporter._ring_plan
            if plan is not None:
                ws = plan.ws
                entry["shape"] = (ws.R, ws.K, ws.S)
                entry["table"] = ws.table.cpu().numpy().copy()
                entry["direct"] = be.pace_score(ws, ws.table, 0, ws.R, 1).records()
                be.synchronize()
            out.append(entry)
        return {"reports": out, "rehomed": int(rings.lib.nvrx_ctx_info(rings.ctx, 5)), "lane_is_none": Detector._lane is None}
    finally:
        Detector.shutdown()
