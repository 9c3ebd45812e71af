"""Worker functions and the scenario of the tests of pace scores per peer group (importable by spawned processes).  The CPU
workers install the checker backend WITH grouped pace scores themselves, as their first statement (``mp_util.run_ranks``
installs the plain one)."""
import pickle

import numpy as np

from pace_workers import ranks_named

RANKS, KERNELS, SLOW_RANK, SAMPLES = 8, 120, 6, 200
SEEDS = (0, 1, 2026)
LAYOUTS = {"block:4": [4, 5, 6, 7], "block:2": [2, 3, 6, 7]}  # layout -> whom the job-wide rule names (the odd stages)
KERNEL_NAMES = tuple(f"kernel_{k:03d}" for k in range(KERNELS))


def scenario_medians(layout, seed=2026, ranks=RANKS, kernels=KERNELS):
    """``[ranks, kernels]`` f32 kernel medians in microseconds of a pipeline job: lognormal kernel times (around 100 us, sigma
    0.5), 1 % noise per entry, the odd stages of ``layout`` (``"block:N"``: stage ``rank // N``) 1.5 x slower in every kernel,
    and rank 6 4 % slower than its stage in every kernel."""
    n = int(layout.partition(":")[2])
    rng = np.random.default_rng(seed)
    base = rng.lognormal(np.log(100.0), 0.5, kernels)
    med = base[None, :] * (1.0 + 0.01 * rng.standard_normal((ranks, kernels)))
    med[(np.arange(ranks) // n) % 2 == 1] *= 1.5
    med[SLOW_RANK] *= 1.04
    return med.astype(np.float32)


def _install_cpu_backend(**kw):
    from nvrx_straggler import backend
    from pace_group_oracle_backend import PaceGroupOracleBackend

    be = PaceGroupOracleBackend(**kw)
    backend.set_backend(be)
    return be


def ring_reports_recorded(rank, world, gather_on_rank0, grouped=True, emulate_fused=False, asynchronous=False):
    """Six ring reports on the checker backend with pace scores and peer groups (``block:2``) on, the pace step per peer group
    or not; a new section appears on the last rank at report 3 and a new kernel on rank 0 at report 5.  Returns the collectives
    this rank issued per report and what the reports said."""
    from tail_workers import record_collectives

    be = _install_cpu_backend(emulate_fused=emulate_fused)
    calls = record_collectives()
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=gather_on_rank0,
                          node_name=f"node{rank}", pace_scores=True, pace_min_ranks=2, peer_groups="block:2",
                          pace_peer_groups=grouped, asynchronous=asynchronous)
    rings = be.make_rings(1, 16, 64)
    rng = np.random.default_rng(100 + rank)
    section_rows = {n: rings.row_for(0, n) for n in ("s0", "s1")}
    kernel_rows = {n: rings.row_for(1, n) for n in ("k0", "k1", "ncclDevKernel_z")}
    out, marks, fused = [], [], []
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
            planned = gen._ring_plan is not None  # (else this report takes the general path and plans the next ones)
            rep = gen.generate_report_from_rings(rings, section_rows, kernel_rows)
            rings.reset()
            marks.append(calls[start:])
            plan = gen._ring_plan
            fused.append(None if not planned or plan is None else bool(plan.fused))
            entry = {"pace": None}
            if rep is not None:
                t = rep.pace_scores()
                entry["pace"] = t
                entry["pickled_same"] = repr(pickle.loads(pickle.dumps(rep)).pace_scores()) == repr(t)
            out.append(entry)
        return {"calls": marks, "reports": out, "fused": fused, "pace_calls": be.pace_calls,
                "pace_group_calls": be.pace_group_calls, "pace_group_args": be.pace_group_args}
    finally:
        gen.close()


# ---- GPU workers (product backend) -------------------------------------------------------------------------------------
def _direct(be, ws, groups, min_ranks, min_peers):
    """What ``backend.pace_group_score`` says of the workspace's table as it stands."""
    return be.pace_group_score(ws, ws.table, groups, 0, ws.R, min_ranks, min_peers).records()


def folded_pace_group(rank, world, layout="block:4", reports=3, asynchronous=False):
    """The scenario through FoldedJob on the product backend (one section, the step, next to the 120 kernel rows): the general
    report, then planned ones.  Per report: what it said, whom the grouped rule names, the table it was computed from (read
    back from the workspace) and what ``backend.pace_group_score`` says of that same table."""
    import torch

    from nvrx_straggler.backend import get_backend
    from nvrx_straggler.folded import FoldedJob

    torch.cuda.set_device(0)
    med = scenario_medians(layout)
    job = FoldedJob(total_ranks=RANKS, section_names=["step"], ring_cap=256, scores_to_compute=("relative_perf_scores",),
                    node_name=f"node{rank}", kernel_names=KERNEL_NAMES, pace_scores=True, peer_groups=layout,
                    pace_peer_groups=True, asynchronous=asynchronous)
    be = get_backend()
    try:
        out = []
        for i in range(reports):
            for lr, r in enumerate(job.logical_ranks()):
                job.load(lr, np.full((1, SAMPLES), med[r].sum(), dtype=np.float32))
                job.load_kernels(lr, np.repeat(med[r][:, None], SAMPLES, axis=1))
            rep = job.report()
            entry = {"pace": rep.pace_scores(), "named": ranks_named(rep.identify_pace_stragglers()),
                     "fused": getattr(job.reporter, "_last_plan_fused", None)}
            plan = job.reporter._ring_plan
            if plan is not None:
                ws = plan.ws
                be.synchronize()
                torch.cuda.synchronize()
                entry["shape"] = (ws.R, ws.K, ws.S)
                entry["table"] = ws.table.cpu().numpy().copy()
                groups = job.reporter._peer_for(ws)
                entry["groups"] = (groups.host.copy(), groups.G, groups.max_size)
                entry["direct"] = _direct(be, ws, groups, min(4, ws.R), 2)
            out.append(entry)
        return out
    finally:
        job.close()


def folded_pace_group_sync_then_async(rank, world, **options):
    """``folded_pace_group`` twice in one process: synchronous reports, then asynchronous ones (each with rings of its own)."""
    return {"sync": folded_pace_group(rank, world, asynchronous=False, **options),
            "async": folded_pace_group(rank, world, asynchronous=True, **options)}


def held_reports(rank, world, windows=5):
    """Reports held across the next two on the same workspace: every window's kernel takes another time, and each report is
    read only after two more were issued.  Four ranks in two groups (``mod:2``: {0, 2} and {1, 3})."""
    import torch

    from nvrx_straggler.folded import FoldedJob

    torch.cuda.set_device(0)
    job = FoldedJob(total_ranks=4, section_names=["step"], ring_cap=64, scores_to_compute=("relative_perf_scores",),
                    kernel_names=("gemm",), pace_scores=True, pace_min_ranks=2, peer_groups="mod:2", pace_peer_groups=True)
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
    """Asynchronous Detector reports with pace scores per peer group (one rank, one group, ``peer_min_ranks=1``), re-homed
    onto the stream their stamps ran on (forced by a 1 us gap): section i of window t holds samples of 10 t + i only, so a pace
    step that read another window's table would show another center.  Per report: what it said, the table it was computed
    from and what ``backend.pace_group_score`` says of that same table."""
    import torch

    from nvrx_straggler import Detector
    from nvrx_straggler.backend import get_backend

    Detector.initialize(scores_to_compute="all", gather_on_rank0=True, node_name="n", asynchronous=True, pace_scores=True,
                        peer_groups="block:1", peer_min_ranks=1, pace_peer_groups=True)
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
                groups = Detector.reporter._peer_for(ws)
                entry["groups"] = (groups.host.copy(), groups.G, groups.max_size)
                entry["direct"] = _direct(be, ws, groups, 1, 1)
                be.synchronize()
            out.append(entry)
        return {"reports": out, "rehomed": int(rings.lib.nvrx_ctx_info(rings.ctx, 5)), "lane_is_none": Detector._lane is None}
    finally:
        Detector.shutdown()
