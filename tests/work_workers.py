"""Worker functions of the work-group tests (importable by spawned processes).  The CPU ones install the checker backend WITH
work groups themselves, as their first statement (``mp_util.run_ranks`` installs the plain one)."""
import json
import pickle

import numpy as np

from peer_workers import flagged

SHARED = tuple(f"gemm_{i}" for i in range(8))
ONLY_STAGE0, ONLY_STAGE1 = ("embed_fwd", "embed_bwd"), ("loss_fwd", "loss_bwd")
KERNELS = SHARED + ONLY_STAGE0 + ONLY_STAGE1
CALLS = (16, 24)  # how often a shared kernel runs per window in stage 0 / stage 1
SLOW_RANK, SLOW = 6, 1.4


def stage_kernels(stage):
    """``{kernel: calls per window}`` of a rank of pipeline stage ``stage``: the shared kernels 1.5 x as often in stage 1, two
    kernels only stage 0 has, two only stage 1."""
    out = {k: CALLS[stage] for k in SHARED}
    out.update({k: 8 for k in (ONLY_STAGE0, ONLY_STAGE1)[stage]})
    return out


def stage_window(r, sections=4, stage=None, seed=3):
    """``(section samples [sections, 9] f32, {kernel: samples f32})`` of logical rank ``r`` of the two-stage job: stage 0 (ranks
    0-3) takes 1000 us a section, stage 1 1500 us; every kernel takes the same time wherever it runs; rank 6 is 1.4 x slower in
    everything; 1 % noise around exact medians."""
    stage = r // 4 if stage is None else stage
    rng = np.random.default_rng(seed * 100 + r)
    slow = SLOW if r == SLOW_RANK else 1.0

    def around(med, n):
        half = (n - 1) // 2
        v = np.concatenate([med * rng.uniform(0.98, 0.999, half), [med], med * rng.uniform(1.001, 1.02, n - 1 - half)])
        return rng.permutation(v).astype(np.float32)

    sec = np.stack([around((1000.0, 1500.0)[stage] * (1 + 0.1 * s) * slow, 9) for s in range(sections)])
    kernels = {k: around((20.0 + 7.0 * i) * slow, n) for i, (k, n) in enumerate(sorted(stage_kernels(stage).items()))}
    return sec, kernels


def _install_cpu_backend(**kw):
    from nvrx_straggler import backend
    from work_oracle_backend import WorkOracleBackend

    be = WorkOracleBackend(**kw)
    backend.set_backend(be)
    return be


def ring_reports_recorded(rank, world, gather_on_rank0, local_ranks=1, emulate_fused=False, asynchronous=False, **options):
    """Six ring reports on the checker backend, ``local_ranks`` logical ranks per process (even logical ranks run three
    ``k_even_*`` kernels, odd ones three ``k_odd_*``); a new section appears on the last rank at report 3 and a new kernel on
    rank 0 at report 5.  Returns the collectives this rank issued per report and what the reports said."""
    from tail_workers import record_collectives

    be = _install_cpu_backend(emulate_fused=emulate_fused)
    calls = record_collectives()
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=gather_on_rank0,
                          node_name=f"node{rank}", asynchronous=asynchronous, **options)
    rings = be.make_rings(local_ranks, 16, 64)
    rng = np.random.default_rng(100 + rank)
    section_rows = {n: rings.row_for(0, n) for n in ("s0", "s1")}
    parity = [f"k_{p}_{x}" for p in ("even", "odd") for x in "abc"]
    kernel_rows = {n: rings.row_for(1, n) for n in ["k0"] + parity + ["ncclDevKernel_z"]}
    out, marks = [], []
    try:
        for i in range(6):
            if i == 2 and rank == world - 1:
                section_rows = dict(section_rows, s_new=rings.row_for(0, "s_new"))
            if i == 4 and rank == 0:
                kernel_rows = dict(kernel_rows, k_new=rings.row_for(1, "k_new"))
            for table in (section_rows, kernel_rows):
                for name, row in table.items():
                    for lr in range(local_ranks):
                        q = rank * local_ranks + lr
                        if name.startswith(("k_odd", "k_even")[q % 2]):
                            continue  # (the other parity's kernels: this logical rank never runs them)
                        rings.push_many(row, rng.lognormal(2.0 + 0.1 * rank, 0.3, 11 + 2 * i).astype(np.float32), lr=lr)
            start = len(calls)
            rep = gen.generate_report_from_rings(rings, section_rows, kernel_rows, local_ranks=local_ranks)
            rings.reset()
            marks.append(calls[start:])
            entry = {"work": None}
            if rep is not None:
                w = rep.work_groups()
                json.dumps({k: v for k, v in w.items() if k in ("singletons", "params", "ranks_with_data")})
                entry["work"] = w
                entry["pickled_same"] = repr(pickle.loads(pickle.dumps(rep)).work_groups()) == repr(w)
                entry["peer"] = rep.peer_scores()
            out.append(entry)
        return {"calls": marks, "reports": out, "work_calls": be.work_calls, "work_args": be.work_args}
    finally:
        gen.close()


# ---- GPU workers (product backend) -------------------------------------------------------------------------------------
def folded_two_stages(rank, world, reports=3, asynchronous=False, sections=4, swap_at=None, hold=False, **options):
    """The two-stage job through FoldedJob on the product backend: the general report, then planned ones.  ``swap_at``: from
    that report on ranks 2 and 5 trade stages (another layout, other groups).  Per report: the work groups, the peer scores and
    both verdicts -- read at once, or (``hold``) only after the last report was issued."""
    from nvrx_straggler.folded import FoldedJob

    job = FoldedJob(total_ranks=8, sections=sections, ring_cap=64, scores_to_compute=("relative_perf_scores",),
                    node_name=f"node{rank}", asynchronous=asynchronous, kernel_names=KERNELS, **options)

    def read(rep):
        if rep is None:
            return None
        return {"work": rep.work_groups(), "peer": rep.peer_scores(), "job_flagged": flagged(rep.identify_stragglers()),
                "peer_flagged": flagged(rep.identify_peer_stragglers())}

    try:
        out, held = [], []
        for i in range(reports):
            for lr, r in enumerate(job.logical_ranks()):
                stage = r // 4
                if swap_at is not None and i >= swap_at and r in (2, 5):
                    stage = 1 - stage
                sec, kernels = stage_window(r, sections, stage)
                job.load(lr, sec)
                for name, values in kernels.items():
                    job.rings.push_many(job._no_kernel_rows[name], values, lr=lr)
            rep = job.report()
            held.append(rep)
            entry = {} if hold else read(rep)
            if entry is not None:
                entry["fused"] = getattr(job.reporter, "_last_plan_fused", None)
            out.append(entry)
        if hold:
            for i in range(reports):  # the oldest first: two more reports were issued on its workspace since
                out[i].update(read(held[i]))
        return out
    finally:
        job.close()
