"""Worker functions of the peer-history tests (importable by spawned processes).  The CPU ones install the checker backend
WITH the peer-score history themselves, as their first statement (``mp_util.run_ranks`` installs the plain one)."""
import numpy as np


def flagged(found):
    """Ranks named anywhere in an ``identify_*stragglers`` result."""
    ranks = set()
    for v in found.values():
        for group in (v.values() if isinstance(v, dict) else [v]):
            ranks |= {s.rank for s in group}
    return sorted(ranks)


def ring_reports_counted(rank, world, gather_on_rank0, reports=5):
    """``reports`` ring reports on the checker backend with a peer history of 4, then as many without: what the history's
    counter said after each report, the step's arguments, the depth each held report showed, and the collectives this rank
    issued per report either way."""
    from nvrx_straggler import backend
    from peer_history_oracle_backend import PeerHistoryOracleBackend
    from tail_workers import record_collectives

    be = PeerHistoryOracleBackend()
    backend.set_backend(be)
    calls = record_collectives()
    from nvrx_straggler.reporting import ReportGenerator

    def run(**options):
        gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=gather_on_rank0, node_name=f"node{rank}",
                              peer_groups="block:2", peer_min_ranks=1, **options)
        rings = be.make_rings(1, 8, 64)
        rows = {n: rings.row_for(0, n) for n in ("s0", "s1")}
        rng = np.random.default_rng(7 + rank)
        n_before, depths, marks = [], [], []
        try:
            for i in range(reports):
                for row in rows.values():
                    rings.push_many(row, rng.lognormal(2.0 + 0.5 * rank, 0.1, 11).astype(np.float32))
                start = len(calls)
                rep = gen.generate_report_from_rings(rings, rows, {})
                rings.reset()
                marks.append(calls[start:])
                state = gen._peer_history
                n_before.append(None if state is None else state.n_before)
                depths.append(rep.peer_history().get("depth") if rep is not None else None)
            return n_before, depths, marks
        finally:
            gen.close()

    n_before, depths, calls_on = run(peer_history=4, peer_trends=True, trend_min_reports=4)
    out = {"n_before": n_before, "depths": depths, "calls_on": calls_on, "peer_history_calls": be.peer_history_calls,
           "peer_calls": be.peer_calls, "args": list(be.peer_history_args)}
    out["calls_off"] = run()[2]
    assert be.peer_history_calls == out["peer_history_calls"]  # (the second run made none)
    return out


# ---- GPU workers (product backend, or the checker for the reference) ------------------------------------------------------
def stage_windows(reports, ranks=8, sections=4, samples=33, seed=41, slow_rank=6, slow_from=4, blip=(1, 2)):
    """``[reports, ranks, sections, samples]`` f32: two stages of 1000 us and 1500 us (the lower and the upper half of the
    ranks), 1 % noise; ``slow_rank`` is 1.4 x slower from report ``slow_from`` on, rank ``blip[0]`` 1.6 x in report
    ``blip[1]`` only."""
    rng = np.random.default_rng(seed)
    x = np.repeat(np.array([1000.0] * (ranks // 2) + [1500.0] * (ranks - ranks // 2)), sections * samples)
    x = x.reshape(1, ranks, sections, samples) * (1.0 + 0.01 * rng.standard_normal((reports, ranks, sections, samples)))
    x[slow_from:, slow_rank] *= 1.4
    x[blip[1], blip[0]] *= 1.6
    return x.astype(np.float32)


def said(rep):
    """What a report says of the peer history: everything the comparison with the reference looks at."""
    src = rep.__dict__.get("_peer_history")
    records = None if src is None else np.array(src.handle.records())  # (before the report builds its dicts and lets go of it)
    return {"peer_history": rep.peer_history(), "peer_trends": rep.peer_trends(),
            "persistent": {k: sorted(flagged({k: v})) if not isinstance(v, dict) else {n: sorted(s.rank for s in g) for n, g in v.items()}
                           for k, v in rep.identify_persistent_peer_stragglers().items()},
            "declining": {k: sorted(flagged({k: v})) if not isinstance(v, dict) else {n: sorted(s.rank for s in g) for n, g in v.items()}
                          for k, v in rep.identify_declining_peer_stragglers().items()},
            "per_report": flagged(rep.identify_peer_stragglers()),
            "records": records}


def folded_reports(rank, world, reports=12, total_ranks=8, asynchronous=False, peer_groups="block:4", gather_on_rank0=True,
                   kernels=False, **options):
    """The two-stage job, ``total_ranks`` logical ranks folded onto ``world`` processes, on whichever backend is installed: the
    general report, then planned ones; the reports are read only after all were issued.  Per report what ``said`` returns
    (``None`` where this rank holds none), and whether the report was planned.  Only the ranks of the slower stage
    have the last section, so that ``peer_groups="auto"`` has something to tell the stages apart by (and the others are
    unrated on it in every report)."""
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator

    sections, names = 5, (("gemm_a", "gemm_b", "norm") if kernels else ())
    local = total_ranks // world
    data = stage_windows(reports, ranks=total_ranks, sections=sections + len(names), slow_rank=total_ranks - 2,
                         slow_from=min(4, reports // 2))
    be = backend.get_backend()
    gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=gather_on_rank0, node_name=f"node{rank}",
                          asynchronous=asynchronous, peer_groups=peer_groups, **options)
    rings = be.make_rings(local, sections + len(names), 64)
    rows = {f"section_{s:03d}": rings.row_for(0, f"section_{s:03d}") for s in range(sections)}
    kernel_rows = {n: rings.row_for(1, n) for n in names}
    try:
        held, planned = [], []
        for i in range(reports):
            for lr in range(local):
                x = data[i, rank * local + lr]
                own = sections if rank * local + lr >= total_ranks // 2 else sections - 1
                for s, row in enumerate(list(rows.values())[:own]):
                    rings.push_many(row, x[s], lr=lr)
                for k, row in enumerate(kernel_rows.values()):
                    rings.push_many(row, x[sections + k] * np.float32(0.3), lr=lr)
            planned.append(gen._ring_plan is not None)
            held.append(gen.generate_report_from_rings(rings, rows, kernel_rows, local_ranks=local))
            rings.reset()
        out = []
        for rep, was_planned in zip(held, planned):
            if rep is None:
                out.append(None)
                continue
            entry = said(rep)
            entry["planned"] = was_planned
            entry["peer_section_relative"] = rep.peer_scores()["section_relative"]
            entry["peer_gpu_relative"] = rep.peer_scores()["gpu_relative"]
            out.append(entry)
        return out
    finally:
        gen.close()
        close = getattr(rings, "close", None)
        if close is not None:
            close()
