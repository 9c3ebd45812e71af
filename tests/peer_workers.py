"""Worker functions of the peer-group score tests (importable by spawned processes).  The CPU ones install the checker
backend WITH peer scores themselves, as their first statement (``mp_util.run_ranks`` installs the plain one)."""
import json
import pickle

import numpy as np


def flagged(found):
    """Ranks named anywhere in an ``identify_*stragglers`` result."""
    ranks = set()
    for v in found.values():
        for group in (v.values() if isinstance(v, dict) else [v]):
            ranks |= {s.rank for s in group}
    return sorted(ranks)


def _install_cpu_backend(**kw):
    from nvrx_straggler import backend
    from peer_oracle_backend import PeerOracleBackend

    be = PeerOracleBackend(**kw)
    backend.set_backend(be)
    return be


def ring_reports_recorded(rank, world, gather_on_rank0, peer_groups="mod:2", local_ranks=1, peer_min_ranks=1,
                          emulate_fused=False, asynchronous=False, **options):
    """Six ring reports on the checker backend, ``local_ranks`` logical ranks per process; a new section appears on the last
    rank at report 3 and a new kernel on rank 0 at report 5.  Returns the collectives this rank issued per report, what the
    reports said and the medians this process's logical ranks pushed."""
    from tail_workers import record_collectives

    be = _install_cpu_backend(emulate_fused=emulate_fused)
    calls = record_collectives()
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=gather_on_rank0,
                          node_name=f"node{rank}", peer_groups=peer_groups, peer_min_ranks=peer_min_ranks,
                          asynchronous=asynchronous, **options)
    rings = be.make_rings(local_ranks, 16, 64)
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
            medians = {}
            for kind, table in (("section", section_rows), ("kernel", kernel_rows)):
                for name, row in table.items():
                    for lr in range(local_ranks):
                        v = rng.lognormal(2.0 + 0.1 * rank, 0.3, 11 + 2 * i).astype(np.float32)  # (odd counts: MED is a sample)
                        rings.push_many(row, v, lr=lr)
                        medians.setdefault(f"{kind}:{name}", []).append(float(np.sort(v)[(v.size - 1) // 2]))
            start = len(calls)
            rep = gen.generate_report_from_rings(rings, section_rows, kernel_rows, local_ranks=local_ranks)
            rings.reset()
            marks.append(calls[start:])
            entry = {"medians": medians, "peer": None}
            if rep is not None:
                t = rep.peer_scores()
                json.dumps({k: v for k, v in t.items() if k not in ("groups", "group_of")})
                entry["peer"] = t
                entry["pickled_same"] = repr(pickle.loads(pickle.dumps(rep)).peer_scores()) == repr(t)
                entry["section_relative"] = {n: dict(v) for n, v in rep.section_relative_perf_scores.items()}
                entry["explained"] = sorted(rep.explain_gpu_scores())
                entry["robust"] = sorted(rep.robust_scores())
                entry["tails"] = sorted(rep.tail_scores())
            out.append(entry)
        return {"calls": marks, "reports": out, "peer_calls": be.peer_calls, "peer_args": be.peer_args}
    finally:
        gen.close()


# ---- GPU workers (product backend) -------------------------------------------------------------------------------------
KERNELS = ("gemm_a", "gemm_b", "norm")


def stage_samples(n=33, noise=0.01, sections=4):
    """``(samples [8, sections + 3, n] f32, medians [8, sections + 3] f32)``: the samples' row medians are
    ``peer_oracle_backend.stage_medians(noise)``; the last three rows are the kernels ``KERNELS`` (0.4, 0.25 and 0.05 of a
    section's time)."""
    from peer_oracle_backend import stage_medians

    med = stage_medians(noise, sections=sections + len(KERNELS))
    med[:, sections:] *= np.array([0.4, 0.25, 0.05])
    med = med.astype(np.float32)
    rng = np.random.default_rng(9)
    half = (n - 1) // 2
    lo = med[:, :, None] * rng.uniform(0.90, 0.999, med.shape + (half,)).astype(np.float32)
    hi = med[:, :, None] * rng.uniform(1.001, 1.10, med.shape + (n - 1 - half,)).astype(np.float32)
    out = np.concatenate([lo, med[:, :, None], hi], axis=2).astype(np.float32)
    rng.permuted(out, axis=2, out=out)
    return out, med


def folded_stages(rank, world, reports=3, asynchronous=False, peer_groups="block:4", sections=4, **options):
    """The two-stage job through FoldedJob on the product backend, ``world`` processes sharing the GPU: the general report,
    then planned ones.  Every report's peer scores, and both verdicts."""
    from nvrx_straggler.folded import FoldedJob

    data, _ = stage_samples(sections=sections)
    job = FoldedJob(total_ranks=8, sections=sections, ring_cap=64, scores_to_compute=("relative_perf_scores",),
                    node_name=f"node{rank}", peer_groups=peer_groups, asynchronous=asynchronous, kernel_names=KERNELS,
                    **options)
    try:
        out = []
        for _ in range(reports):
            for lr, r in enumerate(job.logical_ranks()):
                job.load(lr, data[r, :sections])
                job.load_kernels(lr, data[r, sections:])
            rep = job.report()
            if rep is None:
                out.append(None)
                continue
            t = rep.peer_scores()
            out.append({"peer": t, "job_flagged": flagged(rep.identify_stragglers()),
                        "peer_flagged": flagged(rep.identify_peer_stragglers()),
                        "section_relative": {n: dict(v) for n, v in rep.section_relative_perf_scores.items()},
                        "fused": getattr(job.reporter, "_last_plan_fused", None),
                        "rehomed": int(job.rings.lib.nvrx_ctx_info(job.rings.ctx, 5))})
        return out
    finally:
        job.close()


def folded_stages_sync_then_async(rank, world, **options):
    """``folded_stages`` twice in one process: synchronous reports, then asynchronous ones (each with rings of its own)."""
    import torch

    torch.cuda.set_device(0)
    return {"sync": folded_stages(rank, world, asynchronous=False, **options),
            "async": folded_stages(rank, world, asynchronous=True, **options)}
