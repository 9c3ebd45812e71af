"""Worker functions of the tests of the slack scores per peer group (importable by spawned processes).  The CPU ones install
the checker backend WITH the grouped slack scores themselves, as their first statement (``mp_util.run_ranks`` installs the
plain one)."""
import pickle

import numpy as np

from slack_group_oracle_backend import ALLREDUCE, SENDRECV, STAGE_GEMMS, stage_scenario
from slack_oracle_backend import named


def ring_reports_recorded(rank, world, gather_on_rank0, emulate_fused=False, asynchronous=False, grouped=True, peer_groups="block:2"):
    """Four ring reports on the checker backend, one logical rank per process, ranks in blocks of two doing different work;
    every rank has a compute kernel and an all-reduce whose time depends on the rank.  Returns the collectives this rank
    issued per report and what the reports' slack scores said."""
    from nvrx_straggler import backend
    from slack_group_oracle_backend import SlackGroupOracleBackend
    from tail_workers import record_collectives

    be = SlackGroupOracleBackend(emulate_fused=emulate_fused)
    backend.set_backend(be)
    calls = record_collectives()
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=gather_on_rank0,
                          node_name=f"node{rank}", asynchronous=asynchronous, collective_slack=True, peer_groups=peer_groups,
                          peer_min_ranks=1, slack_min_ranks=2, slack_peer_groups=grouped)
    rings = be.make_rings(1, 16, 64)
    rng = np.random.default_rng(100 + rank)
    gemm = STAGE_GEMMS[(rank // 2) % 2]
    section_rows = {n: rings.row_for(0, n) for n in ("s0", "s1")}
    kernel_rows = {gemm: rings.row_for(1, gemm), ALLREDUCE: rings.row_for(1, ALLREDUCE)}
    out, marks = [], []
    try:
        for i in range(4):
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
                "group_calls": be.slack_group_calls, "group_args": be.slack_group_args}
    finally:
        gen.close()


STAGES_2_4 = (0, 0, 1, 1, 1, 1)


def gpu_stage_ranks(rank, world, gather_on_rank0, peer_groups=STAGES_2_4, late_rank=4):
    """GPU worker, ``world`` = 3 gloo processes sharing one device with two logical ranks each: 6 logical ranks in stages of 2
    and 4, the stage scenario's kernels; ``late_rank`` arrives 300 us late.  Two reports (the general path, then the planned
    one)."""
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator

    be = backend.get_backend()
    gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=gather_on_rank0, node_name=f"node{rank}",
                          collective_slack=True, peer_groups=peer_groups, slack_peer_groups=True)
    local = len(STAGES_2_4) // world
    rings = be.make_rings(local, 8, 256)
    section_rows = {"step": rings.row_for(0, "step")}
    kernel_rows = {k: rings.row_for(1, k) for k in STAGE_GEMMS + (ALLREDUCE, SENDRECV)}
    step, gemm, allreduce, bubble = stage_scenario(STAGES_2_4, late_rank)
    out = []
    try:
        for _ in range(2):
            for lr in range(local):
                r = rank * local + lr
                rings.push_many(section_rows["step"], step[r], lr=lr)
                rings.push_many(kernel_rows[STAGE_GEMMS[STAGES_2_4[r]]], gemm, lr=lr)
                rings.push_many(kernel_rows[ALLREDUCE], allreduce[r], lr=lr)
                rings.push_many(kernel_rows[SENDRECV], bubble[r], lr=lr)
            rep = gen.generate_report_from_rings(rings, section_rows, kernel_rows, local_ranks=local)
            rings.reset()
            entry = {"held": rep is not None}
            if rep is not None:
                entry["slack"] = rep.slack_scores()
                entry["named"] = named(rep.identify_slack_stragglers())
            out.append(entry)
        return out
    finally:
        gen.close()
        rings.close()
