"""Worker functions of the robust-score tests (importable by spawned processes).  The CPU ones install the checker backend
WITH robust scores themselves, as their first statement (``mp_util.run_ranks`` installs the plain one)."""
import json
import pickle

import numpy as np

SLOW_RANK, FAST_RANK = 3, 5


def scenario_medians(ranks=8, sections=64):
    """The issue's job: ``ranks`` x ``sections`` medians around 1000 with 1 % noise, rank 5 at 0.6 x the time (it skips work),
    rank 3 at 1.3 x (the straggler)."""
    rng = np.random.default_rng(2024)
    med = 1000.0 * (1.0 + 0.01 * rng.standard_normal((ranks, sections)))
    med[FAST_RANK] *= 0.6
    med[SLOW_RANK] *= 1.3
    return med.astype(np.float32)


def scenario_samples(n=33):
    """[8, 64, n] samples whose row medians are ``scenario_medians()``: the median in the middle, a spread around it."""
    med = scenario_medians()
    rng = np.random.default_rng(5)
    half = (n - 1) // 2
    lo = med[:, :, None] * rng.uniform(0.90, 0.999, med.shape + (half,)).astype(np.float32)
    hi = med[:, :, None] * rng.uniform(1.001, 1.10, med.shape + (n - 1 - half,)).astype(np.float32)
    out = np.concatenate([lo, med[:, :, None], hi], axis=2).astype(np.float32)
    rng.permuted(out, axis=2, out=out)
    return out


def flagged(found):
    """Ranks named anywhere in an ``identify_*stragglers`` result."""
    ranks = {s.rank for s in found["straggler_gpus_relative"]}
    for v in found["straggler_sections_relative"].values():
        ranks |= {s.rank for s in v}
    return sorted(ranks)


def _install_cpu_backend(**kw):
    from nvrx_straggler import backend
    from robust_oracle_backend import RobustOracleBackend

    be = RobustOracleBackend(**kw)
    backend.set_backend(be)
    return be


def ring_reports_recorded(rank, world, gather_on_rank0, robust=True, emulate_fused=False, asynchronous=False,
                          kernel_attribution=0, tail_quantile=0.0):
    """Six ring reports on the checker backend; a new section appears on the last rank at report 3 and a new kernel on rank 0
    at report 5.  Returns the collectives this rank issued per report and what the reports said."""
    from tail_workers import record_collectives

    be = _install_cpu_backend(emulate_fused=emulate_fused)
    calls = record_collectives()
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=gather_on_rank0,
                          node_name=f"node{rank}", robust_scores=robust, robust_min_ranks=2, asynchronous=asynchronous,
                          kernel_attribution=kernel_attribution, tail_quantile=tail_quantile)
    rings = be.make_rings(1, 16, 64)
    rng = np.random.default_rng(100 + rank)
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
                    v = rng.lognormal(2.0 + 0.1 * rank, 0.3, 11 + 3 * i + rank).astype(np.float32)
                    rings.push_many(row, v)
                    pushed[f"{kind}:{name}"] = v.tolist()
            start = len(calls)
            rep = gen.generate_report_from_rings(rings, section_rows, kernel_rows)
            rings.reset()
            marks.append(calls[start:])
            entry = {"pushed": pushed, "robust": None}
            if rep is not None:
                t = rep.robust_scores()
                entry["robust"] = t
                entry["pickled_same"] = repr(pickle.loads(pickle.dumps(rep)).robust_scores()) == repr(t)
                entry["explained"] = sorted(rep.explain_gpu_scores())
                entry["tails"] = sorted(rep.tail_scores())
            out.append(entry)
        return {"calls": marks, "reports": out, "robust_calls": be.robust_calls, "robust_args": be.robust_args}
    finally:
        gen.close()


# ---- GPU workers (product backend) -------------------------------------------------------------------------------------
def folded_scenario(rank, world, kernel_attribution=0, reports=3):
    """The scenario through FoldedJob on the product backend, ``world`` processes sharing the GPU."""
    from nvrx_straggler.folded import FoldedJob

    data = scenario_samples()
    job = FoldedJob(total_ranks=8, sections=64, ring_cap=64, scores_to_compute=("relative_perf_scores",),
                    node_name=f"node{rank}", kernel_attribution=kernel_attribution, robust_scores=True)
    try:
        out = []
        for _ in range(reports):  # the general report, then planned ones
            for lr, r in enumerate(job.logical_ranks()):
                job.load(lr, data[r])
            rep = job.report()
            if rep is None:
                out.append(None)
                continue
            t = rep.robust_scores()
            json.dumps(t)
            out.append({"robust": t, "median_flagged": flagged(rep.identify_stragglers()),
                        "robust_flagged": flagged(rep.identify_robust_stragglers()),
                        "explained": sorted(rep.explain_gpu_scores())})
        return out
    finally:
        job.close()


def ring_windows_asynchronous(rank, world, windows=40):
    """Device rings + an ASYNCHRONOUS ReportGenerator in one process, one logical rank, 8 sections x 256 samples, a new
    window every report.  Returns what every report's robust scores said and how often their one copy-out had run at each
    point."""
    import torch

    from nvrx_straggler import _native
    from nvrx_straggler.backend import get_backend
    from nvrx_straggler.reporting import ReportGenerator

    torch.cuda.set_device(0)
    be = get_backend()
    S, n = 8, 256
    rings = be.make_rings(1, S, n)
    gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=True, node_name="n", asynchronous=True, robust_scores=True)
    names = [f"sec{s}" for s in range(S)]
    rows = {name: rings.row_for(_native.KIND_SECTION, name) for name in names}
    no_kernels = {}
    calls = [0]
    inner = be.robust_copy_out

    def counted(t):
        calls[0] += 1
        return inner(t)

    be.robust_copy_out = counted
    rng = np.random.default_rng(11)
    host = rng.lognormal(np.log(100.0), 0.3, (windows, S, n)).astype(np.float32)
    host[1::2] *= np.float32(10.0)
    dev = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    try:
        out = []
        for w in range(windows):
            for s, name in enumerate(names):
                rings.push_device(rows[name], dev[w, s])
            be.synchronize()
            torch.cuda.synchronize()
            rep = gen.generate_report_from_rings(rings, rows, no_kernels)
            rings.reset()
            at_return = calls[0]
            rep.identify_stragglers()
            dict(rep.section_relative_perf_scores)
            before = calls[0]
            t = rep.robust_scores()
            after_first = calls[0]
            rep.robust_scores()
            out.append({"robust": t, "copy_outs": (at_return, before, after_first, calls[0])})
        return {"reports": out, "samples": host, "names": names, "enqueue_only": gen.enqueue_only()}
    finally:
        gen.close()
        rings.close()


def detector_one_process(rank, world, entries=12):
    """Detector with the option on, region timing (stamps), one profile_cuda section, one process."""
    import torch

    from nvrx_straggler import Detector

    Detector.initialize(scores_to_compute="all", gather_on_rank0=True, node_name=f"node{rank}", robust_scores=True)
    try:
        x = torch.randn(512, 512, device="cuda")
        x = x / x.norm()
        out = []
        for _ in range(3):
            for _i in range(entries):
                with Detector.detection_section("work", profile_cuda=True):
                    y = x @ x
                    x = y / y.norm()
            torch.cuda.synchronize()
            rep = Detector.generate_report()
            out.append({"robust": rep.robust_scores(), "flagged": flagged(rep.identify_robust_stragglers())})
        return {"windows": out, "lane_is_none": Detector._lane is None, "on": Detector.reporter.robust_scores}
    finally:
        Detector.shutdown()
