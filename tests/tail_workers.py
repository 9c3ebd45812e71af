"""Worker functions of the tail-score tests (importable by spawned processes).  The CPU ones install the checker backend
WITH tails themselves, as their first statement (``mp_util.run_ranks`` installs the plain one)."""
import json
import os
import pickle
import time

import numpy as np


def _install_cpu_backend(**kw):
    from nvrx_straggler import backend
    from tail_oracle_backend import TailOracleBackend

    be = TailOracleBackend(**kw)
    backend.set_backend(be)
    return be


def headline_data():
    """The issue's table: 8 ranks x 64 sections x 10 000 samples, rank 3 slow by 1.5 x on a random 10 % of its samples."""
    rng = np.random.default_rng(7)
    base = rng.lognormal(np.log(1000.0), 0.02, (8, 64, 10000)).astype(np.float32)
    slow = rng.random((64, 10000)) < 0.10
    base[3] = np.where(slow, base[3] * np.float32(1.5), base[3])
    return base


def record_collectives():
    """Wrap the collectives a report may issue; returns the list they append ``(kind, payload length)`` to.  Row gathers
    carry their element count; an object gather's pickled size legitimately differs by rank (each sends its own names),
    so only that it happened is recorded."""
    from nvrx_straggler import dist_utils, name_mapper

    calls = []
    rows, objs, flag = dist_utils.all_gather_rows, dist_utils.all_gather_object, dist_utils.is_all_true

    def all_gather_rows(send, table, group=None):
        calls.append(("rows", int(send.numel())))
        return rows(send, table, group)

    def all_gather_object(obj, group=None):
        calls.append(("object", 0))
        return objs(obj, group)

    def is_all_true(f, group=None):
        calls.append(("flag", 1))
        return flag(f, group)

    dist_utils.all_gather_rows = all_gather_rows
    dist_utils.all_gather_object = name_mapper.all_gather_object = all_gather_object
    dist_utils.is_all_true = name_mapper.is_all_true = is_all_true
    return calls


def ring_reports_recorded(rank, world, gather_on_rank0, q=0.9, emulate_fused=False, asynchronous=False):
    """Six ring reports on the checker backend; a new section appears on the last rank at report 3 and a new kernel on rank 0
    at report 5.  Returns the collectives this rank issued, per report what was pushed, and what the report said."""
    be = _install_cpu_backend(emulate_fused=emulate_fused)
    calls = record_collectives()
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=gather_on_rank0,
                          node_name=f"node{rank}", tail_quantile=q, asynchronous=asynchronous)
    rings = be.make_rings(1, 16, 64)
    rng = np.random.default_rng(100 + rank)
    section_rows = {n: rings.row_for(0, n) for n in ("s0", "s1")}
    kernel_rows = {n: rings.row_for(1, n) for n in ("k0", "ncclDevKernel_z")}
    out = []
    marks = []
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
            entry = {"pushed": pushed, "tails": None}
            if rep is not None:
                t = rep.tail_scores()
                json.dumps(t)
                entry["tails"] = t
                entry["rel"] = dict(rep.gpu_relative_perf_scores)
                entry["pickled_same"] = json.dumps(pickle.loads(pickle.dumps(rep)).tail_scores()) == json.dumps(t)
            out.append(entry)
        return {"calls": marks, "reports": out, "tail_local_calls": be.tail_local_calls, "tail_score_calls": be.tail_score_calls}
    finally:
        gen.close()


# ---- GPU workers (product backend) -------------------------------------------------------------------------------------
def folded_headline(rank, world, kernel_attribution=0, q=0.95):
    """The headline shape through FoldedJob on the product backend, ``world`` processes sharing the GPU."""
    from nvrx_straggler.folded import FoldedJob

    data = headline_data()
    job = FoldedJob(total_ranks=8, sections=64, ring_cap=10000, scores_to_compute=("relative_perf_scores",),
                    node_name=f"node{rank}", kernel_attribution=kernel_attribution, tail_quantile=q)
    try:
        out = []
        for _ in range(3):  # the general report, then planned ones
            for lr, r in enumerate(job.logical_ranks()):
                job.load(lr, data[r])
            rep = job.report()
            if rep is None:
                out.append(None)
                continue
            found = rep.identify_stragglers()
            tail_found = rep.identify_tail_stragglers()
            explain = rep.explain_gpu_scores()
            t = rep.tail_scores()
            out.append({
                "tails": t,
                "median_flagged": sorted(s.rank for s in found["straggler_gpus_relative"])
                + sorted(s.rank for v in found["straggler_sections_relative"].values() for s in v),
                "tail_sections": {n: sorted(s.rank for s in v) for n, v in tail_found["straggler_sections_relative"].items()},
                "tail_gpus": sorted(s.rank for s in tail_found["straggler_gpus_relative"]),
                "explained": sorted(explain),
            })
        return out
    finally:
        job.close()


def _gpu_spin(x, n):
    for _ in range(n):
        x = x @ x
        x = x / x.norm()
    return x


def detector_peer_with_tails(rank, world, q=0.9, reports=3):
    """Two processes with NVRX_EXCHANGE=peer in the environment and the option on: the reports run on c10d."""
    import logging

    import torch

    from nvrx_straggler import Detector

    lines = []

    class Grab(logging.Handler):
        def emit(self, record):
            lines.append(record.getMessage())

    logging.getLogger("nvrx_straggler.reporting").addHandler(Grab())
    Detector.initialize(scores_to_compute="all", gather_on_rank0=True, node_name=f"node{rank}", tail_quantile=q)
    try:
        x = torch.randn(256, 256, device="cuda")
        x = x / x.norm()
        out = []
        for _ in range(reports):
            for i in range(12):
                with Detector.detection_section("work", profile_cuda=True):
                    _gpu_spin(x, 40 if (rank == 1 and i % 3 == 0) else 4)
            torch.cuda.synchronize()
            rep = Detector.generate_report()
            if rep is not None:
                out.append({"tails": rep.tail_scores(), "rel": dict(rep.gpu_relative_perf_scores),
                            "kernels": sorted(rep.local_kernel_summaries)})
        info = dict(Detector.reporter.exchange_info)
        return {"reports": out, "route": info.get("route", ""), "mode": info.get("mode", ""),
                "direct": Detector.reporter._direct is not None,
                "ignored_lines": [m for m in lines if "NVRX_EXCHANGE" in m and "tail_quantile" in m]}
    finally:
        Detector.shutdown()


def ring_windows_written_from_another_stream(rank, world, asynchronous, windows=40, q=0.9):
    """Device rings + ReportGenerator.generate_report_from_rings in one process, one logical rank, 8 sections x 4096 samples.
    Right after each report call returns, the NEXT window's samples -- ten times larger or smaller -- are appended with
    ``nvrx_ring_push_device`` from a stream of the test's own.  Returns every report's section tails, the windows' samples,
    and how often the tails' one copy-out had run at each point."""
    import torch

    from nvrx_straggler import _native
    from nvrx_straggler.backend import get_backend
    from nvrx_straggler.reporting import ReportGenerator

    torch.cuda.set_device(0)
    be = get_backend()
    S, n = 8, 4096
    rings = be.make_rings(1, S, n)
    gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=True, node_name="n", asynchronous=asynchronous, tail_quantile=q)
    names = [f"sec{s}" for s in range(S)]
    rows = {name: rings.row_for(_native.KIND_SECTION, name) for name in names}
    no_kernels = {}
    calls = [0]
    inner = be.tails_copy_out

    def counted(t):
        calls[0] += 1
        return inner(t)

    be.tails_copy_out = counted
    rng = np.random.default_rng(11)
    host = rng.lognormal(np.log(100.0), 0.3, (windows, S, n)).astype(np.float32)
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
        held = None
        for w in range(windows):
            rep = gen.generate_report_from_rings(rings, rows, no_kernels)
            rings.reset()
            if w + 1 < windows:
                push(w + 1)  # at once, from another stream, over the slots the report's kernels read
            at_return = calls[0]
            rep.identify_stragglers()
            dict(rep.section_relative_perf_scores)
            before = calls[0]
            t = rep.tail_scores()
            after_first = calls[0]
            rep.tail_scores()
            out.append({"section_tails": {k: v[0] for k, v in t["section_tails"].items()},
                        "section_relative": {k: v[0] for k, v in t["section_relative"].items()},
                        "copy_outs": (at_return, before, after_first, calls[0])})
            other.synchronize()  # the next report reads the next window
            held = rep
        return {"reports": out, "samples": host, "names": names}
    finally:
        gen.close()
        rings.close()


def detector_bursty_section(rank, world, q=0.9, entries=24):
    """Detector, region timing (stamps), two profile_cuda sections; ``bursty`` does three times the GPU work on every 4th
    entry.  One process is its own reference."""
    import torch

    from nvrx_straggler import Detector, Statistic

    Detector.initialize(scores_to_compute="all", gather_on_rank0=True, node_name=f"node{rank}", tail_quantile=q)
    try:
        x = torch.randn(2048, 2048, device="cuda")
        x = x / x.norm()
        out = []
        for _ in range(2):
            for i in range(entries):
                with Detector.detection_section("steady", profile_cuda=True):
                    _gpu_spin(x, 4)
                with Detector.detection_section("bursty", profile_cuda=True):
                    _gpu_spin(x, 12 if i % 4 == 3 else 4)
            torch.cuda.synchronize()
            rep = Detector.generate_report()
            t = rep.tail_scores()
            out.append({"tails": t, "med": {k: v[Statistic.MED] for k, v in rep.local_kernel_summaries.items()},
                        "tail_stragglers": rep.identify_tail_stragglers()["straggler_gpus_relative"] == set()})
        return {"windows": out, "lane_is_none": Detector._lane is None}
    finally:
        Detector.shutdown()
