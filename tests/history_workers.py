"""Worker functions and scenarios of the score-history tests (importable by spawned processes).  The CPU ones install the
checker backend WITH the score history themselves, as their first statement (``mp_util.run_ranks`` installs the plain one)."""
import pickle

import numpy as np

RANKS, REPORTS, SEED = 8, 20, 17
ONCE_RANK, ONCE_REPORT, ONCE_FACTOR = 2, 6, 1.6      # slow in one report only
STAYS_RANK, STAYS_FROM, STAYS_FACTOR = 5, 10, 1.45   # slow from that report on
SECTIONS = ("fwd", "bwd")


def scenario_window(report, samples=9):
    """``[RANKS, len(SECTIONS), samples]`` f32 of one report window of the issue's scenario: 8 ranks around 1000 with 1 %
    noise; rank 2 is 1.6 x slower in report 6 only, rank 5 is 1.45 x slower from report 10 on."""
    rng = np.random.default_rng([SEED, report])
    x = 1000.0 * (1.0 + 0.01 * rng.standard_normal((RANKS, len(SECTIONS), samples)))
    if report == ONCE_REPORT:
        x[ONCE_RANK] *= ONCE_FACTOR
    if report >= STAYS_FROM:
        x[STAYS_RANK] *= STAYS_FACTOR
    return x.astype(np.float32)


def run_scenario(be, reports=REPORTS, **options):
    """The scenario through a gathering generator on the active backend ``be``, 8 logical ranks in one process.  Returns the
    reports, unread."""
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=True, node_name="n", **options)
    rings = be.make_rings(RANKS, len(SECTIONS), 16)
    rows = {n: rings.row_for(0, n) for n in SECTIONS}
    out = []
    try:
        for i in range(reports):
            w = scenario_window(i)
            for lr in range(RANKS):
                for s, n in enumerate(SECTIONS):
                    rings.push_many(rows[n], w[lr, s], lr=lr)
            out.append(gen.generate_report_from_rings(rings, rows, {}, local_ranks=RANKS))
            rings.reset()
    finally:
        gen.close()
    return out


def ranks_of(found):
    """Ranks named anywhere in an ``identify_*stragglers`` result."""
    ranks = set()
    for v in found.values():
        for group in (v.values() if isinstance(v, dict) else [v]):
            ranks |= {s.rank for s in group}
    return sorted(ranks)


def _install_cpu_backend(**kw):
    from history_oracle_backend import HistoryOracleBackend
    from nvrx_straggler import backend

    be = HistoryOracleBackend(**kw)
    backend.set_backend(be)
    return be


def ring_reports_recorded(rank, world, gather_on_rank0, history=8, emulate_fused=False, asynchronous=False, **options):
    """Six ring reports on the checker backend; a new section appears on the last rank at report 3.  Returns the collectives
    this rank issued per report and what the reports' histories said."""
    from tail_workers import record_collectives

    be = _install_cpu_backend(emulate_fused=emulate_fused)
    calls = record_collectives()
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=gather_on_rank0,
                          node_name=f"node{rank}", score_history=history, persistence_min_reports=2 if history else 3,
                          asynchronous=asynchronous, **options)
    rings = be.make_rings(1, 16, 64)
    rng = np.random.default_rng(100 + rank)
    section_rows = {n: rings.row_for(0, n) for n in ("s0", "s1")}
    kernel_rows = {"k0": rings.row_for(1, "k0")}
    out, marks = [], []
    try:
        for i in range(6):
            if i == 2 and rank == world - 1:
                section_rows = dict(section_rows, s_new=rings.row_for(0, "s_new"))
            for table in (section_rows, kernel_rows):
                for row in table.values():
                    rings.push_many(row, rng.lognormal(2.0 + 0.4 * rank, 0.05, 11 + rank).astype(np.float32))
            start = len(calls)
            rep = gen.generate_report_from_rings(rings, section_rows, kernel_rows)
            rings.reset()
            marks.append(calls[start:])
            entry = {"history": None}
            if rep is not None:
                t = rep.score_history()
                entry["history"] = t
                entry["pickled_same"] = repr(pickle.loads(pickle.dumps(rep)).score_history()) == repr(t)
                entry["persistent"] = ranks_of(rep.identify_persistent_stragglers())
                entry["flagged"] = ranks_of(rep.identify_stragglers())
            out.append(entry)
        return {"calls": marks, "reports": out, "history_calls": be.history_calls, "history_args": be.history_args}
    finally:
        gen.close()
