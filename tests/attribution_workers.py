"""Worker functions of the kernel-attribution tests (importable by spawned processes).  The CPU ones install the checker
backend WITH attribution themselves, as their first statement (``mp_util.run_ranks`` installs the plain one)."""
import json
import os
import pickle
import time

import numpy as np

from workers import _summ, report_to_plain


def _install_cpu_backend():
    from attribution_oracle_backend import AttributionOracleBackend
    from nvrx_straggler import backend

    backend.set_backend(AttributionOracleBackend())


def _mapper_ids(gen):
    m = gen.name_mapper if gen._exchanged() else gen._private_mapper
    return dict(m.kernel_name_to_id)


def scoring_scenario_attributed(rank, world, scenario, top_n=16, cpu=True):
    """One golden scenario through ReportGenerator(kernel_attribution=top_n) on the dict-input path: per step the plain report,
    its explanation, and the same explanation after a pickle round trip."""
    if cpu:
        _install_cpu_backend()
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(scenario["scores_to_compute"], gather_on_rank0=scenario["gather_on_rank0"], node_name=f"node{rank}",
                          kernel_attribution=top_n)
    try:
        out = []
        for step in scenario["steps"]:
            sec, ker = step[rank]
            rep = gen.generate_report(_summ(sec), _summ(ker))
            if rep is None:
                out.append(None)
                continue
            ex = rep.explain_gpu_scores()
            again = pickle.loads(pickle.dumps(rep)).explain_gpu_scores()
            out.append({"report": report_to_plain(rep), "explain": ex, "pickled_same": json.dumps(again) == json.dumps(ex),
                        "kernel_ids": _mapper_ids(gen)})
        return out
    finally:
        gen.close()


def scoring_scenarios_attributed_batch(rank, world, scenarios, top_n=16, cpu=True):
    return [scoring_scenario_attributed(rank, world, sc, top_n, cpu) for sc in scenarios]


def _gpu_spin(x, n):
    for _ in range(n):
        x = x @ x
        x = x / x.norm()
    return x


def detector_two_windows(rank, world, asynchronous=False, top_n=3, slow_factor=8, counting=False):
    """Detector, region timing, two profile_cuda sections; in the second window section ``b``'s GPU work is ``slow_factor``
    times longer.  Returns both windows' explanations and scores; ``counting``: also how often the attribution's one wait
    (``HipBackend.attribution_copy_out``) had run before / after the first ``explain_gpu_scores()`` of the second report."""
    import torch

    from nvrx_straggler import Detector
    from nvrx_straggler import backend as backend_mod

    Detector.initialize(scores_to_compute="all", gather_on_rank0=True, node_name=f"node{rank}", asynchronous=asynchronous,
                        kernel_attribution=top_n)
    try:
        be = backend_mod.get_backend()
        calls = [0]
        if counting:
            inner = be.attribution_copy_out

            def counted(attr):
                calls[0] += 1
                return inner(attr)

            be.attribution_copy_out = counted
        x = torch.randn(256, 256, device="cuda")
        x = x / x.norm()
        out = []
        for window, (na, nb) in enumerate(((4, 4), (4, 4 * slow_factor))):
            for _ in range(12):
                with Detector.detection_section("a", profile_cuda=True):
                    _gpu_spin(x, na)
                with Detector.detection_section("b", profile_cuda=True):
                    _gpu_spin(x, nb)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rep = Detector.generate_report()
            dt = time.perf_counter() - t0
            if rep is None:
                out.append(None)
                continue
            before_scores = calls[0]
            stragglers = rep.identify_stragglers()
            indiv = dict(rep.gpu_individual_perf_scores)
            rel = dict(rep.gpu_relative_perf_scores)
            before_explain = calls[0]
            ex = rep.explain_gpu_scores()
            out.append({"explain": ex, "indiv": indiv, "rel": rel, "kernels": sorted(rep.local_kernel_summaries),
                        "copy_outs": (before_scores, before_explain, calls[0]), "report_s": dt,
                        "flagged": sorted(s.rank for s in stragglers["straggler_gpus_individual"])})
        return {"windows": out, "lane_is_none": Detector._lane is None}
    finally:
        Detector.shutdown()


def detector_peer_two_ranks(rank, world, top_n=3, reports=4):
    """Two processes, ring path over the in-stream route the environment selects (peer windows): rank 1's GPU section is
    several times longer.  Rank 0's explanations of every report, with its scores."""
    import torch

    from nvrx_straggler import Detector

    Detector.initialize(scores_to_compute="all", gather_on_rank0=True, node_name=f"node{rank}", kernel_attribution=top_n)
    try:
        x = torch.randn(256, 256, device="cuda")
        x = x / x.norm()
        out = []
        for _ in range(reports):
            for _ in range(8):
                with Detector.detection_section("work", profile_cuda=True):
                    _gpu_spin(x, 4 if rank == 0 else 40)
            torch.cuda.synchronize()
            rep = Detector.generate_report()
            if rep is not None:
                out.append({"explain": rep.explain_gpu_scores(), "rel": dict(rep.gpu_relative_perf_scores),
                            "indiv": dict(rep.gpu_individual_perf_scores)})
        info = dict(Detector.reporter.exchange_info)
        return {"reports": out, "route": info.get("route", ""), "fused": Detector.reporter._ring_plan is not None
                and Detector.reporter._ring_plan.fused and Detector.reporter._direct is not None}
    finally:
        Detector.shutdown()
