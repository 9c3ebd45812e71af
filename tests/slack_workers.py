"""Worker functions of the slack-score tests (importable by spawned processes).  The CPU ones install the checker backend
WITH slack scores themselves, as their first statement (``mp_util.run_ranks`` installs the plain one)."""
import pickle

import numpy as np

from slack_oracle_backend import ALLREDUCE, GEMM, named, scenario


def _install_cpu_backend(**kw):
    from nvrx_straggler import backend
    from slack_oracle_backend import SlackOracleBackend

    be = SlackOracleBackend(**kw)
    backend.set_backend(be)
    return be


def ring_reports_recorded(rank, world, gather_on_rank0, emulate_fused=False, asynchronous=False, slack=True, tail=0.0):
    """Six ring reports on the checker backend, every rank with a compute kernel and an all-reduce whose time depends on the
    rank; a new section appears on the last rank at report 2, a new COLLECTIVE kernel on rank 0 at report 4.  Returns the
    collectives this rank issued per report and what the reports' slack scores said."""
    from tail_workers import record_collectives

    be = _install_cpu_backend(emulate_fused=emulate_fused)
    calls = record_collectives()
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=gather_on_rank0,
                          node_name=f"node{rank}", asynchronous=asynchronous, collective_slack=slack, tail_quantile=tail)
    rings = be.make_rings(1, 16, 64)
    rng = np.random.default_rng(100 + rank)
    section_rows = {n: rings.row_for(0, n) for n in ("s0", "s1")}
    kernel_rows = {"k0": rings.row_for(1, "k0"), ALLREDUCE: rings.row_for(1, ALLREDUCE)}
    out, marks = [], []
    try:
        for i in range(6):
            if i == 2 and rank == world - 1:
                section_rows = dict(section_rows, s_new=rings.row_for(0, "s_new"))
            if i == 4 and rank == 0:
                kernel_rows = dict(kernel_rows, ncclDevKernel_new=rings.row_for(1, "ncclDevKernel_new"))
            for table in (section_rows, kernel_rows):
                for name, row in table.items():
                    base = 200.0 + 100.0 * rank if name == ALLREDUCE else 50.0
                    rings.push_many(row, (base * (1.0 + 0.01 * rng.standard_normal(12))).astype(np.float32))
            start = len(calls)
            rep = gen.generate_report_from_rings(rings, section_rows, kernel_rows)
            rings.reset()
            marks.append(calls[start:])
            entry = {"slack": None}
            if rep is not None:
                s = rep.slack_scores()
                entry["slack"] = s
                entry["pickled_same"] = repr(pickle.loads(pickle.dumps(rep)).slack_scores()) == repr(s)
                entry["named"] = named(rep.identify_slack_stragglers())
            out.append(entry)
        return {"calls": marks, "reports": out, "local_calls": be.slack_local_calls, "score_calls": be.slack_score_calls,
                "lists": be.slack_lists, "args": be.slack_args, "route": gen.exchange_info.get("route", "")}
    finally:
        gen.close()


def gpu_rank_late(rank, world, gather_on_rank0, late_rank=1):
    """GPU worker, ``world`` gloo processes sharing one device: one logical rank each, the scenario's compute kernel, step
    section and all-reduce; ``late_rank`` arrives 300 us late.  Two reports (the general path, then the planned one)."""
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator

    be = backend.get_backend()
    gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=gather_on_rank0, node_name=f"node{rank}",
                          collective_slack=True)
    rings = be.make_rings(1, 4, 256)
    section_rows = {"step": rings.row_for(0, "step")}
    kernel_rows = {GEMM: rings.row_for(1, GEMM), ALLREDUCE: rings.row_for(1, ALLREDUCE)}
    step, gemm, coll = scenario(late_rank, 300.0, ranks=world)
    out = []
    try:
        for _ in range(2):
            rings.push_many(section_rows["step"], step)
            rings.push_many(kernel_rows[GEMM], gemm)
            rings.push_many(kernel_rows[ALLREDUCE], coll[rank])
            rep = gen.generate_report_from_rings(rings, section_rows, kernel_rows)
            rings.reset()
            entry = {"held": rep is not None}
            if rep is not None:
                entry["slack"] = rep.slack_scores()
                entry["named"] = named(rep.identify_slack_stragglers())
                entry["flagged"] = named(rep.identify_stragglers())
            out.append(entry)
        return out
    finally:
        gen.close()
        rings.close()
