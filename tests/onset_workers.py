"""Worker functions of the onset-score tests (importable by spawned processes).  The CPU ones install the checker backend
WITH onsets themselves, as their first statement (``mp_util.run_ranks`` installs the plain one)."""
import json
import pickle

import numpy as np

from tail_workers import record_collectives

RANKS, SECTIONS, SAMPLES = 8, 4, 2000
STEP_RANK, BURST_RANK, STEP_AT = 3, 5, 1400  # the step: 1.5 x from 70 % of the window on, 600 samples before its end


def _install_cpu_backend(**kw):
    from nvrx_straggler import backend
    from onset_oracle_backend import OnsetOracleBackend

    be = OnsetOracleBackend(**kw)
    backend.set_backend(be)
    return be


def headline_data():
    """8 ranks x 4 sections x 2000 samples around 1000 with 1 % noise; rank 3 is 1.5 x slower from sample 1400 on, rank 5
    on a random 10 % of its samples."""
    rng = np.random.default_rng(17)
    base = (1000.0 * (1.0 + 0.01 * rng.standard_normal((RANKS, SECTIONS, SAMPLES)))).astype(np.float32)
    base[STEP_RANK, :, STEP_AT:] *= np.float32(1.5)
    bursts = rng.random((SECTIONS, SAMPLES)) < 0.10
    base[BURST_RANK] = np.where(bursts, base[BURST_RANK] * np.float32(1.5), base[BURST_RANK])
    return base


def summarise(rep):
    """What the headline checks look at, as plain data."""
    found = rep.identify_stragglers()
    onset_found = rep.identify_onset_stragglers()
    return {
        "onsets": rep.onset_scores(),
        "section_relative": {n: dict(v) for n, v in rep.section_relative_perf_scores.items()},
        "median_flagged": sorted(s.rank for s in found["straggler_gpus_relative"])
        + sorted(s.rank for v in found["straggler_sections_relative"].values() for s in v),
        "onset_sections": {n: sorted(s.rank for s in v) for n, v in onset_found["straggler_sections_relative"].items()},
        "onset_gpus": sorted(s.rank for s in onset_found["straggler_gpus_relative"]),
    }


def ring_reports_recorded(rank, world, gather_on_rank0, emulate_fused=False, asynchronous=False, tail_quantile=0.0):
    """Six ring reports on the checker backend; rank 1's section s0 steps up by 1.5 x two thirds of the way through every
    window; a new section appears on the last rank at report 3 and a new kernel on rank 0 at report 5.  Returns the
    collectives this rank issued, per report what was pushed, and what the report said."""
    be = _install_cpu_backend(emulate_fused=emulate_fused)
    calls = record_collectives()
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=gather_on_rank0,
                          node_name=f"node{rank}", onset_detection=True, asynchronous=asynchronous, tail_quantile=tail_quantile)
    rings = be.make_rings(1, 16, 64)
    rng = np.random.default_rng(200 + rank)
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
                    n = 12 + 8 * i + rank  # (12..54: the first windows are too short for an onset)
                    v = (10.0 * (1.0 + 0.01 * rng.standard_normal(n))).astype(np.float32)
                    if rank == 1 and name == "s0":
                        v[2 * n // 3:] *= np.float32(1.5)
                    rings.push_many(row, v)
                    pushed[f"{kind}:{name}"] = v.tolist()
            start = len(calls)
            rep = gen.generate_report_from_rings(rings, section_rows, kernel_rows)
            rings.reset()
            marks.append(calls[start:])
            entry = {"pushed": pushed, "onsets": None}
            if rep is not None:
                t = rep.onset_scores()
                json.dumps(t)
                entry["onsets"] = t
                entry["tails"] = rep.tail_scores()
                entry["flagged"] = {n: sorted(s.rank for s in v)
                                    for n, v in rep.identify_onset_stragglers()["straggler_sections_relative"].items()}
                entry["pickled_same"] = json.dumps(pickle.loads(pickle.dumps(rep)).onset_scores()) == json.dumps(t)
            out.append(entry)
        return {"calls": marks, "reports": out, "onset_local_calls": be.onset_local_calls,
                "onset_score_calls": be.onset_score_calls, "onset_enable_calls": be.onset_enable_calls}
    finally:
        gen.close()


# ---- GPU workers (product backend) -------------------------------------------------------------------------------------
def folded_headline(rank, world, tail_quantile=0.0):
    """The headline shape through FoldedJob on the product backend, ``world`` processes sharing the GPU."""
    from nvrx_straggler.folded import FoldedJob

    data = headline_data()
    job = FoldedJob(total_ranks=RANKS, sections=SECTIONS, ring_cap=SAMPLES, scores_to_compute=("relative_perf_scores",),
                    node_name=f"node{rank}", onset_detection=True, tail_quantile=tail_quantile)
    try:
        out = []
        for _ in range(3):  # the general report, then planned ones
            for lr, r in enumerate(job.logical_ranks()):
                job.load(lr, data[r])
            rep = job.report()
            out.append(None if rep is None else dict(summarise(rep), tails=rep.tail_scores()))
        return out
    finally:
        job.close()


def ring_windows_written_from_another_stream(rank, world, asynchronous, windows=12):
    """Device rings + ReportGenerator.generate_report_from_rings in one process, one logical rank, 8 sections x 4096 samples,
    every window with a step at a place of its own.  Right after each report call returns, the NEXT window's samples -- ten
    times larger or smaller, stepping elsewhere -- are appended with ``nvrx_ring_push_device`` from a stream of the test's
    own.  Returns every report's section onsets, the windows' samples, and how often the onsets' one copy-out had run."""
    import torch

    from nvrx_straggler import _native
    from nvrx_straggler.backend import get_backend
    from nvrx_straggler.reporting import ReportGenerator

    torch.cuda.set_device(0)
    be = get_backend()
    S, n = 8, 4096
    rings = be.make_rings(1, S, n)
    gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=True, node_name="n", asynchronous=asynchronous,
                          onset_detection=True)
    names = [f"sec{s}" for s in range(S)]
    rows = {name: rings.row_for(_native.KIND_SECTION, name) for name in names}
    no_kernels = {}
    calls = [0]
    inner = be.onsets_copy_out

    def counted(t):
        calls[0] += 1
        return inner(t)

    be.onsets_copy_out = counted
    rng = np.random.default_rng(12)
    host = (100.0 * (1.0 + 0.01 * rng.standard_normal((windows, S, n)))).astype(np.float32)
    steps = rng.integers(n // 10, n - n // 10, (windows, S))
    for w in range(windows):
        for s in range(S):
            host[w, s, steps[w, s]:] *= np.float32(1.5)
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
            t = rep.onset_scores()
            after_first = calls[0]
            rep.onset_scores()
            out.append({"section_onsets": {k: v[0] for k, v in t["section_onsets"].items()},
                        "section_relative": {k: v[0] for k, v in t["section_relative"].items()},
                        "copy_outs": (at_return, before, after_first, calls[0])})
            other.synchronize()  # the next report reads the next window
        return {"reports": out, "samples": host, "names": names, "steps": steps}
    finally:
        gen.close()
        rings.close()


def wrapped_ring(rank, world, ring_cap=64):
    """One and a half ring capacities of samples pushed into 64-deep rings, the step inside the surviving window; a second
    window that does not wrap follows.  Returns the onsets and what was pushed."""
    import torch

    from nvrx_straggler import _native
    from nvrx_straggler.backend import get_backend
    from nvrx_straggler.reporting import ReportGenerator

    torch.cuda.set_device(0)
    be = get_backend()
    rings = be.make_rings(1, 4, ring_cap)
    gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=True, node_name="n", onset_detection=True)
    names = [f"sec{s}" for s in range(4)]
    rows = {name: rings.row_for(_native.KIND_SECTION, name) for name in names}
    rng = np.random.default_rng(13)
    try:
        out = []
        for pushes in (ring_cap * 3 // 2, ring_cap, ring_cap * 2 + 5, ring_cap - 9):
            pushed = (10.0 * (1.0 + 0.01 * rng.standard_normal((4, pushes)))).astype(np.float32)
            for s, name in enumerate(names):
                pushed[s, pushes - 10 - 7 * s:] *= np.float32(1.5)  # 10, 17, 24, 31 samples before the end
                rings.push_many(rows[name], pushed[s])
            rep = gen.generate_report_from_rings(rings, rows, {})
            rings.reset()
            out.append({"onsets": rep.onset_scores()["section_onsets"], "pushed": pushed})
        return {"windows": out, "names": names}
    finally:
        gen.close()
        rings.close()
