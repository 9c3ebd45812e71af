#!/usr/bin/env python3
"""Benchmark of the straggler-scoring hot path on MI355X: generate_report() latency.

Workload (BASELINE.json, metric "generate_report() us ... 8 ranks x 64 sections x 10k samples"):
8 logical ranks x 64 sections x 10 000 f32 timing samples per report, ring capacity 10 000 on both
sides, relative + individual scores, gather_on_rank0.  With N GPUs each process holds 8/N logical
ranks (strong scaling, total work fixed); N=1 folds the whole job onto one GPU (512 rows, 20.48 MB),
N=8 is the production shape (one rank per GPU, 2.56 MB each).  A "step" is one collective
generate_report(): re-arm resident samples -> flush (scatter kernel) -> statistics kernel -> one
all-gather of the exchange rows (RCCL when N>1) -> score kernel -> one D2H of the results, host
waits.  Inputs are resident in HBM before the timed region starts.

    python bench.py --gpus 1 --steps 200 --warmup 20
    python bench.py --gpus N --steps K --warmup W          (no launcher: spawns its own N ranks, one per GPU)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W
    python bench.py --gpus 1 --steps K --warmup W --full   (every leg below as well)
    python bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR

`value` is the time from calling generate_report() to holding the flagged-straggler set: every timed step keeps its
Report and calls identify_stragglers() on it (rank 0), which waits for and copies the scores / flags out of the result
block; `report_read` adds what building the six dict mappings of that report costs on the host, and
`us_per_report_fully_read` is the sum (the reference's generate_report returns populated dicts, reporting.py:535-545).

A plain run sets up, warms up, times the K steps and prints the headline fields of the line; `--dump-outputs DIR` writes
what the last timed step returned (see _dump_outputs).  Everything else below runs only with `--full`.

Prints ONE JSON line on rank 0 (see the driver contract); extra objects (--full):
  roofline     -- the statistics kernel (k_row_stats) against the HBM roofline: algorithmic bytes =
                  local_ranks * 64 * 10000 * 4 per launch, duration from hipEvent pairs recorded
                  around every launch on the launch stream during a second, instrumented pass of the
                  same K steps (the headline pass runs without the extra event records).
  per_step_overhead -- BASELINE.json's second figure (config #4): the real Detector around a fixed
                  bf16 matmul workload with a hipEvent pair per entry and a collective report EVERY
                  step; % = (t_with - t_without) / t_without, A/B blocks alternating in one process.
  host_inputs  -- the PCIe-inclusive figure (never `value`): the same report when the 8 x 64 x 10 000 samples start in
                  pageable HOST memory and are handed over per logical rank ([64, 10000] f32 arrays -> one H2D copy +
                  one strided device-to-device append of the whole matrix each) before the report runs; N=1 only, a few repetitions.
  cpu_baseline -- the reference's CPU path restated in Python (oracle/, kind "port"), timed on this host: the whole job
                  as 8 gloo processes (one per rank, 8 cores): per report torch.tensor(deque) + 5 torch reductions per
                  section, the flag / MIN all-reduces, scores, gather to rank 0; the all_gather_object of the summary
                  dicts is timed next to it; the single-rank, no-collective figure is kept as a sub-object.
"""
import argparse
import ctypes
import gc
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
for _p in (REPO, os.path.join(REPO, "nvidia-resiliency-ext_amd"), os.path.join(REPO, "tests", "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
# a benchmark must not sit out c10d's 30 minutes if an exchange route misbehaves on a box nobody has seen yet
os.environ.setdefault("NVRX_REPORT_TIMEOUT_S", "60")

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

TOTAL_RANKS = 8
SECTIONS = 64
SAMPLES = 10_000
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6300 GB/s achievable

def _port_vs_reference():
    """How the port's timing relates to the REAL reference's: measured where both exist (the build container -- a Python
    reference cannot travel to the GPU box), both 8-process gloo jobs in the same run, by tools/port_vs_reference_timing.py;
    the committed fixture is read here, nothing is typed in."""
    try:
        with open(os.path.join(REPO, "tests", "golden", "port_vs_reference.json")) as f:
            return json.load(f)
    except Exception as e:  # noqa: BLE001
        return {"error": f"{type(e).__name__}: {e}"}


def _cpu_baseline(reps: int):
    """Reference CPU path, restated (oracle.ref_port_*), on a bounded sample; rank 0, N=1 only."""
    import collections

    import synth
    from oracle import oracle

    torch.set_num_threads(1)
    x = synth.stress_samples(0, SECTIONS, SAMPLES)
    # the reference holds Python floats in deques (straggler.py:80-83, :343)
    deques = {synth.section_name(s): collections.deque(x[s].astype(np.float64).tolist(), maxlen=SAMPLES) for s in range(SECTIONS)}
    t_sum = []
    summ = None
    for _ in range(reps):
        t0 = time.perf_counter()
        summ = oracle.ref_port_section_summaries(deques)
        t_sum.append(time.perf_counter() - t0)
    per_rank = [{n: dict(v) for n, v in summ.items()} for _ in range(TOTAL_RANKS)]
    port = oracle.RefPortReportGenerator(TOTAL_RANKS)
    t_sc = []
    for _ in range(max(reps, 5)):
        t0 = time.perf_counter()
        port.generate_reports(per_rank, [{} for _ in range(TOTAL_RANKS)])
        t_sc.append(time.perf_counter() - t0)
    # C oracle (sorted-copy statistics) for information
    counts = np.full(SECTIONS, SAMPLES, dtype=np.uint32)
    t0 = time.perf_counter()
    for _ in range(5):
        oracle.rows_stats(x, counts)
    t_c = (time.perf_counter() - t0) / 5
    summaries_us = float(np.median(t_sum)) * 1e6
    scoring_us = float(np.median(t_sc)) * 1e6 / TOTAL_RANKS
    single = {
        "value": round(summaries_us + scoring_us, 1),
        "unit": "us",
        "cores": 1,
        "kind": "port",
        "sample": f"1 rank x {SECTIONS} sections x {SAMPLES} samples from Python deques: torch.tensor + 5 torch reductions "
                  f"per section (median of {reps} reps) + dict scoring of {TOTAL_RANKS} simulated ranks / {TOTAL_RANKS}; "
                  "no collectives",
        "summaries_us": round(summaries_us, 1),
        "scoring_us_per_rank": round(scoring_us, 1),
        "c_oracle_stats_us": round(t_c * 1e6, 1),
        "host_cpus": os.cpu_count(),
    }
    # the whole job on the host cores: 8 processes (one per rank, one torch thread each) on gloo, doing what the
    # reference does per report -- summaries, flag + MIN all-reduce, scores, gather to rank 0 -- and, timed separately,
    # the all_gather_object of the summary dicts that BASELINE.json's wording names
    try:
        from oracle import port_mp

        mp_reps = max(5, min(20, reps // 3))
        r = port_mp.run(world=TOTAL_RANKS, sections=SECTIONS, samples=SAMPLES, reps=mp_reps)
    except Exception as e:  # noqa: BLE001  (the single-rank figure still stands)
        single["gloo_job_error"] = str(e)[-300:]
        return single
    pvr = _port_vs_reference()
    ratio = (pvr.get("job_8_gloo_ranks") or {}).get("ratio_port_over_reference")
    return {
        "value": round(r["report_us"], 1),
        "unit": "us",
        "cores": TOTAL_RANKS,
        "kind": "port",
        "sample": f"{TOTAL_RANKS} gloo ranks (one process and one torch thread each) x {SECTIONS} sections x {SAMPLES} samples from "
                  f"Python deques: per report torch.tensor + 5 torch reductions per section, flag + MIN all-reduce, scores, "
                  f"gather to rank 0; max over ranks of the per-rank median of {mp_reps} reports",
        "summaries_us": round(r["summaries_us"], 1),
        "exchange_scoring_us": round(r["exchange_scoring_us"], 1),
        "all_gather_object_of_summaries_us": round(r["all_gather_object_us"], 1),
        "single_rank_no_collectives": single,
        "host_cpus": os.cpu_count(),
        # the reference is Python and cannot travel to the GPU box, so what is timed HERE is the port; the port against the real
        # reference -- both as 8-process gloo jobs, same run, same inputs -- was measured where both exist (fixture)
        "port_vs_reference_measured_in_the_build_container": pvr,
        "reference_equivalent_us": None if not ratio else round(r["report_us"] / ratio, 1),
        "reference_equivalent_note": "this host's port figure / (port / reference measured in the build container): an estimate, not a measurement",
    }


def _per_step_overhead(world: int, rank: int, steps: int, blocks: int, asynchronous: bool = False):
    """BASELINE.json config #4: the real ``Detector`` around a fixed GPU workload (10 x 4096^3 bf16
    matmul), ``profile_cuda=True`` (hipEvent pair per entry), individual scores, a collective
    ``generate_report()`` EVERY step.  A/B blocks of ``steps`` steps alternate in the same process;
    overhead = (t_with - t_without) / t_without on the per-step medians of the blocks."""
    from nvrx_straggler import Detector

    x = torch.randn(4096, 4096, dtype=torch.bfloat16, device="cuda")

    def work():
        y = x
        for _ in range(10):
            y = torch.matmul(x, y)
        return y

    def sync_all():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    Detector.initialize(scores_to_compute=["individual_perf_scores"], gather_on_rank0=True, node_name=f"node{rank}",
                        asynchronous=asynchronous)
    held = [None]
    try:
        def step_with():
            with Detector.detection_section("train_step", profile_cuda=True):
                work()
            rep = Detector.generate_report()
            if asynchronous:
                # the report of step t is consumed during step t+1 (one-step-late detection); it is read for real
                prev, held[0] = held[0], rep
                if prev is not None:
                    prev.identify_stragglers()
            elif rep is not None:
                rep.identify_stragglers()
            return rep

        for _ in range(10):
            work()
            step_with()
        def step_sections_only():
            # what the training loop pays between two reports (production reports once a minute, S/straggler.py:125): the
            # GPU-timed section alone -- two stamp kernels on the step's stream, one staged host sample
            with Detector.detection_section("train_step", profile_cuda=True):
                work()

        t_without, t_with, t_sections = [], [], []
        legs = [(t_without, work), (t_with, step_with)] + ([] if asynchronous else [(t_sections, step_sections_only)])
        for blk in range(blocks):
            # the legs take turns in a rotating order, so that a clock that ramps or a box that warms up over the run does
            # not favour the leg that always comes last
            for acc, fn in legs[blk % len(legs):] + legs[:blk % len(legs)]:
                sync_all()
                t0 = time.perf_counter()
                for _ in range(steps):
                    fn()
                sync_all()
                acc.append((time.perf_counter() - t0) / steps)
                if fn is step_sections_only:
                    Detector.generate_report()  # empties the rings (not timed)
    finally:
        Detector.shutdown()
    a, b = float(np.median(t_without)), float(np.median(t_with))
    c = float(np.median(t_sections)) if t_sections else a
    t = torch.tensor([a, b, c], dtype=torch.float64, device="cuda")
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    a, b, c = t.tolist()
    extra = {} if asynchronous else {
        "sections_only_pct": round((c - a) / a * 100.0, 3), "sections_only_added_us_per_step": round((c - a) * 1e6, 1),
        "sections_only_note": "the same loop with the GPU-timed section but NO report: what a step pays between two reports at "
                              "production cadence (one report per ~60 s, S/straggler.py:125; reference claim: < 1 %)"}
    return {
        **extra,
        "pct": round((b - a) / a * 100.0, 3),
        "step_ms_without": round(a * 1e3, 4),
        "step_ms_with": round(b * 1e3, 4),
        "added_us_per_step": round((b - a) * 1e6, 1),
        "steps_per_block": steps,
        "blocks": blocks,
        "workload": "Detector.detection_section(profile_cuda=True) around 10 x matmul(4096^2, bf16) + generate_report() "
                    "every step, individual_perf_scores, gather_on_rank0"
                    + (", asynchronous=True: report t is enqueued at step t and read (identify_stragglers) during step t+1"
                       if asynchronous else ""),
    }


def _cadence_leg(reports: int, job=None):
    """Reports at the cadence production uses (S/straggler.py:125 reports every ~60 s; BASELINE config #2: one report
    per 100 training steps): between two reports the GPU runs 100 steps of 10 x matmul(4096^2, bf16), so every report
    meets an idle detector stream and caches / TLBs / kernarg lines that the training work has evicted.  Each report
    is timed on its own, call -> flagged set in hand, after the step's own device synchronisation (a training loop
    that logs its loss has one; without it the figure would be the GPU's backlog, not the report).

    ``job`` None: the real ``Detector`` with config #2's four sections (two of them GPU-timed), synchronous and
    asynchronous.  ``job`` given: the headline workload (8 x 64 x 10 000 resident samples) reported at that cadence."""
    from nvrx_straggler import Detector

    x = torch.randn(4096, 4096, dtype=torch.bfloat16, device="cuda")

    def work(n):
        y = x
        for _ in range(n):
            y = torch.matmul(x, y)
        return y

    def summary(t):
        a = np.asarray(t, dtype=np.float64) / 1e3
        return {"us_median": round(float(np.median(a)), 2), "us_p95": round(float(np.percentile(a, 95)), 2),
                "us_mean": round(float(a.mean()), 2), "us_max": round(float(a.max()), 2), "reports": len(t)}

    if job is not None:
        t = []
        for i in range(reports + 2):
            for _ in range(100):
                work(10)
            torch.cuda.synchronize()
            t0 = time.perf_counter_ns()
            job.rearm(SAMPLES)
            job.report().identify_stragglers()
            if i >= 2:
                t.append(time.perf_counter_ns() - t0)
        out = summary(t)
        out["workload"] = (f"the headline report ({TOTAL_RANKS} x {SECTIONS} x {SAMPLES} resident samples) once per 100 steps of "
                           "10 x matmul(4096^2, bf16); each report timed alone, call -> flagged set")
        return out

    out = {}
    for asynchronous in (False, True):
        Detector.initialize(scores_to_compute="all", gather_on_rank0=True, node_name="node0", asynchronous=asynchronous)
        try:
            t, t_late = [], []
            held = None
            for i in range(reports + 2):
                for _ in range(100):
                    with Detector.detection_section("data", profile_cuda=False):
                        pass
                    with Detector.detection_section("forward", profile_cuda=True):
                        work(4)
                    with Detector.detection_section("backward", profile_cuda=True):
                        work(6)
                    with Detector.detection_section("optimizer", profile_cuda=False):
                        pass
                torch.cuda.synchronize()
                t0 = time.perf_counter_ns()
                rep = Detector.generate_report()
                if not asynchronous:
                    rep.identify_stragglers()
                t1 = time.perf_counter_ns()
                if asynchronous and held is not None:
                    held.identify_stragglers()  # the previous report, read 100 steps after it was enqueued
                t2 = time.perf_counter_ns()
                held = rep
                if i >= 2:
                    t.append(t1 - t0)
                    t_late.append(t2 - t1)
            key = "asynchronous" if asynchronous else "synchronous"
            out[key] = summary(t)
            if asynchronous:
                out[key]["read_one_interval_later_us_median"] = round(float(np.median(t_late)) / 1e3, 2)
        finally:
            Detector.shutdown()
    out["workload"] = ("Detector with 4 sections per step (2 GPU-timed), 100 steps of 10 x matmul(4096^2, bf16) between reports "
                       "(BASELINE config #2 cadence); each generate_report() timed alone after the step's device "
                       "synchronisation: synchronous = call -> identify_stragglers() returned; asynchronous = the enqueue, "
                       "the report is read at the next report")
    return out


def _per_kernel_leg(reports: int = 12):
    """Per-kernel mode at the scale of the reference's own sizing (tests/straggler/unit/test_data_shared.py:62-66): K
    kernel keys x 100 durations per report.  The dispatch records are synthetic (tracing 400 000 real launches per report
    is not a benchmark step) and take the tracer's NATIVE path: a feeder thread plays the rocprofiler-sdk callback thread
    and hands batches of ~1100 records (what a 256 KB SDK buffer holds) to ``nvrx_ktrace_feed`` -> key cache -> sink ->
    ``nvrx_ring_push_staged`` while the 'training' thread sleeps; the training thread's part of a report is ``harvest()``
    (``nvrx_ktrace_sync``: a counter comparison, no record is touched) and then one report over the K kernel rows."""
    import threading

    from nvrx_straggler import ktrace
    from nvrx_straggler.reporting import ReportGenerator

    out = {}
    for K in (256, 4096):
        ktrace.KernelTraceProfiler._live = None
        prof = ktrace.KernelTraceProfiler(statsMaxLenPerKernel=128, max_keys=K)
        gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=True, node_name="node0")
        try:
            rng = np.random.default_rng(K)
            base = (1 << 52) + (K << 20)
            for k in range(K):
                ktrace.feed_kernel_name(base + k, f"bench_kernel_{k:04d}")
            d = np.zeros(K * 100, dtype=ktrace.DISPATCH_DTYPE)
            d["kernel_id"] = base + rng.permutation(np.repeat(np.arange(K, dtype=np.uint64), 100))
            d["workgroup"], d["grid"], d["start_ns"] = (256, 1, 1), (256 * 64, 1, 1), 1000
            d["end_ns"] = 1000 + (rng.lognormal(3.0, 0.3, K * 100) * 1000.0).astype(np.uint64)
            rings = prof._rings
            no_sections = {}  # the same object every report: the generator's cached plan stays valid
            t_feed, t_in, t_rep = [], [], []

            def feeder():
                t0 = time.perf_counter_ns()
                for lo in range(0, d.size, 1100):
                    ktrace.feed(d[lo:lo + 1100])
                t_feed.append(time.perf_counter_ns() - t0)

            for i in range(reports + 2):
                th = threading.Thread(target=feeder)
                th.start()
                th.join()                       # (the window's kernels have all finished: nothing left to wait for)
                t0 = time.perf_counter_ns()
                missing = prof.harvest(wait=True)
                t1 = time.perf_counter_ns()
                rep = gen.generate_report_from_rings(rings, no_sections, rings.kernel_row_names)
                score = rep.gpu_relative_perf_scores[0]
                t2 = time.perf_counter_ns()
                rings.reset()
                assert missing == 0
                if i >= 2:
                    t_in.append(t1 - t0)
                    t_rep.append(t2 - t1)
            assert abs(score - 1.0) < 1e-6 and len(rings.kernel_row_names) == K
            out[f"K{K}"] = {"records_per_report": int(d.size), "ingest_us_median": round(float(np.median(t_in)) / 1e3, 2),
                            "report_us_median": round(float(np.median(t_rep)) / 1e3, 1),
                            "tracer_thread_us_per_window": round(float(np.median(t_feed[2:])) / 1e3, 1),
                            "tracer_thread_ns_per_record": round(float(np.median(t_feed[2:])) / d.size, 1)}
        finally:
            gen.close()
            prof.close()
            ktrace.KernelTraceProfiler._live = None
    out["workload"] = ("K kernel keys x 100 durations per report, fed as dispatch records through the tracer's native path by a "
                       "feeder thread (the SDK callback thread's part: key cache -> sink -> staged ring appends, a scatter launch "
                       "per 4096 samples); ingest_us = what the TRAINING thread does at report time (harvest = "
                       "nvrx_ktrace_sync), report_us = one report over the K kernel rows with its GPU score read; round 4: "
                       "K256 85.7 + 30.1 us, K4096 1310 + 196 us with the ingest on the training thread in Python")
    return out


def _kernels_mode_child(mode: str = "kernels"):
    """``python bench.py --child kernels_mode`` (``--child stamp_mode``: the same legs on region stamps, as the comparison): the legs that need PER-KERNEL tracing, in a fresh interpreter -- the tracer
    registers with rocprofiler-sdk before the HIP runtime starts, and the bench's main process has selected its device long
    before.  Prints one JSON object.  This is the mode every multi-rank job runs in (``ktrace.timing_mode``).

    * ``per_step_overhead_kernels`` -- BASELINE.json's second figure in that mode: a step with a realistic dispatch count
      (10 pre-norm transformer layers, d_model 2048, 8 x 1024 tokens, bf16, forward + backward + SGD: > 500 kernel dispatches,
      GPU-bound so the host runs ahead) inside ONE ``detection_section(profile_cuda=True)``.  Legs, A/B blocks alternating in
      one process, medians over blocks: no detector / section every step, no report (production cadence between reports) at
      ``profiling_interval`` 1 and 10 / a synchronous report EVERY step / an asynchronous report every step.  The reference's
      claim for kernel profiling: < 1 % (docs/source/straggler_det/usage_guide.rst:169).
    * ``report_at_cadence_kernels`` -- one report per 100 of those steps, each timed alone after the step's own device
      synchronisation: synchronous (call -> flagged set) and asynchronous (the enqueue; read one interval later)."""
    os.environ["NVRX_GPU_TIMING"] = mode
    import nvrx_straggler  # noqa: F401  (registers the tracer: nothing has touched HIP yet)
    from nvrx_straggler import Detector, ktrace

    torch.cuda.set_device(0)
    torch.manual_seed(0)
    d_model, layers, batch, seq = 2048, 10, 8, 1024
    blocks = torch.nn.ModuleList([torch.nn.TransformerEncoderLayer(d_model, 16, 4 * d_model, dropout=0.0, batch_first=True,
                                                                   norm_first=True) for _ in range(layers)])
    blocks = blocks.to("cuda", torch.bfloat16)
    opt = torch.optim.SGD(blocks.parameters(), lr=1e-6, foreach=True)
    x = torch.randn(batch, seq, d_model, device="cuda", dtype=torch.bfloat16)

    def train_step():
        h = x
        for blk in blocks:
            h = blk(h)
        h.float().square().mean().backward()
        opt.step()
        opt.zero_grad(set_to_none=True)

    for _ in range(3):
        train_step()
    torch.cuda.synchronize()
    out = {"python": "%d.%d.%d" % sys.version_info[:3]}

    def timed(fn, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps

    def overhead_legs(interval, steps, rounds, budget=0.0):
        """``budget`` 0: kernels traced on every ``interval``-th entry whatever it costs (the reference's behaviour); None: the
        package's default (``kernel_trace_budget_pct`` 1.0) -- the loop then calls ``generate_report_if_interval_elapsed()``
        after every step, as the reference's example and the PTL callback do, so that the first 17 iterations calibrate."""
        Detector.initialize(scores_to_compute="all", gather_on_rank0=True, node_name="node0", profiling_interval=interval,
                            **({} if budget is None else {"kernel_trace_budget_pct": budget}))
        try:
            def with_section():
                with Detector.detection_section("train_step", profile_cuda=True):
                    train_step()
                if budget is None:
                    Detector.generate_report_if_interval_elapsed()   # (one report per 60 s: none inside the timed blocks)

            if budget is None:
                for _ in range(20):
                    with_section()                                   # the interval tracker's 16 timed iterations: tracing on / off

            def with_report():
                with_section()
                Detector.generate_report().identify_stragglers()

            for _ in range(3):
                with_report()
            dispatches = 0
            for _ in range(interval * Detector._trace_every):        # (one of these entries is a traced one)
                c0 = ktrace.counters()
                with_section()
                Detector.cupti_manager.harvest(wait=True)
                dispatches = max(dispatches, ktrace.counters()["enqueued"] - c0["enqueued"])
            Detector.generate_report()
            legs = [("without", train_step), ("section", with_section)] + ([("report_every_step", with_report)] if interval == 1 else [])
            acc = {k: [] for k, _ in legs}
            for r in range(rounds):
                for name, fn in legs[r % len(legs):] + legs[:r % len(legs)]:
                    acc[name].append(timed(fn, steps))
                    if name == "section":
                        Detector.generate_report()   # empties the rings (not timed)
            # PAIRED differences: every round times all legs back to back, so the round's own "without" is the reference of its
            # other legs -- clock / thermal drift over the run (which moved the unpaired figure between 0.3 and 2.2 % from one
            # box to the next) cancels inside a round; the median over rounds and the spread are reported
            base = np.asarray(acc["without"])

            def paired(name):
                d = (np.asarray(acc[name]) - base) / base * 100.0
                return {"pct_median": round(float(np.median(d)), 3), "pct_min": round(float(d.min()), 3), "pct_max": round(float(d.max()), 3),
                        "added_us_per_step_median": round(float(np.median(np.asarray(acc[name]) - base)) * 1e6, 1)}

            sec = paired("section")
            res = {"profiling_interval": interval, "kernel_trace_budget_pct": Detector.kernel_trace_budget_pct,
                   "kernel_trace_cost_pct_measured_by_the_calibration": None if Detector.kernel_trace_cost_pct is None else round(Detector.kernel_trace_cost_pct, 3),
                   "kernels_traced_on_every_nth_entry": interval * Detector._trace_every,
                   "dispatches_traced_per_profiled_step": int(dispatches),
                   "step_ms_without": round(float(np.median(base)) * 1e3, 4),
                   "section_every_step_no_report_pct": sec["pct_median"], "section_every_step_no_report": sec}
            if "report_every_step" in acc:
                rep_ = paired("report_every_step")
                res["report_every_step_pct"] = rep_["pct_median"]
                res["report_every_step"] = rep_
            return res
        finally:
            Detector.shutdown()

    steps, rounds = (10, 14) if mode == "kernels" else (10, 8)
    try:
        o1 = overhead_legs(1, steps, rounds)
        o10 = overhead_legs(10, steps, 8) if mode == "kernels" else o1
        odef = overhead_legs(1, steps, rounds, budget=None) if mode == "kernels" else o1
        out["per_step_overhead_kernels"] = {
            # what a job gets WITHOUT touching a setting: Detector.initialize() defaults (profiling_interval 1, kernel_trace_budget_pct
            # 1.0), the reference's loop (a section around the step, generate_report_if_interval_elapsed() after it)
            "default_settings": odef,
            "pct": odef["section_every_step_no_report_pct"],
            "kernels_traced_on_every_nth_entry": odef["kernels_traced_on_every_nth_entry"],
            "dispatches_traced_per_profiled_step": odef["dispatches_traced_per_profiled_step"],
            # the same with the budget off (kernel_trace_budget_pct=0: every entry traced, the reference's behaviour)
            "profiling_interval_1": o1, "profiling_interval_10": o10,
            "pct_budget_off_profiling_interval_1": o1["section_every_step_no_report_pct"],
            "pct_at_profiling_interval_10": o10["section_every_step_no_report_pct"],
            "steps_per_block": steps, "blocks": rounds, "counters": ktrace.counters(),
            "workload": f"{layers} x TransformerEncoderLayer(d_model {d_model}, 16 heads, ffn {4 * d_model}, pre-norm, bf16), batch {batch} x "
                        f"{seq} tokens, forward + backward + SGD inside ONE detection_section(profile_cuda=True), NVRX_GPU_TIMING={mode} "
                        "(kernels: every dispatch of a traced entry recorded by name); pct = section every step, no report (what a step pays "
                        "between two reports) at the DEFAULT settings, where the tracing budget thins tracing to every n-th entry; "
                        "report_every_step_pct = a synchronous generate_report() + identify_stragglers() after every step"}
    except Exception as e:  # noqa: BLE001
        out["per_step_overhead_kernels"] = {"error": f"{type(e).__name__}: {str(e)[-300:]}"}

    def cadence(asynchronous, reports):
        Detector.initialize(scores_to_compute="all", gather_on_rank0=True, node_name="node0", asynchronous=asynchronous)
        try:
            t, t_late, t_harvest, stages, lanes = [], [], [], [], 0
            clk = (ctypes.c_double * 8)()
            wclk = (ctypes.c_double * 2)()
            held = None
            mgr = Detector.cupti_manager
            plain_harvest = mgr.harvest

            def timed_harvest(wait=True):  # the training thread's share of the tracer's work at report time
                h0 = time.perf_counter_ns()
                r = plain_harvest(wait)
                t_harvest.append(time.perf_counter_ns() - h0)
                return r

            mgr.harvest = timed_harvest
            for i in range(reports + 2):
                for _ in range(40):
                    with Detector.detection_section("train_step", profile_cuda=True):
                        train_step()
                torch.cuda.synchronize()
                lane = Detector._lane
                n_h = len(t_harvest)
                t0 = time.perf_counter_ns()
                rep = Detector.generate_report()
                tg = time.perf_counter_ns()
                if not asynchronous:
                    rep.identify_stragglers()
                t1 = time.perf_counter_ns()
                if asynchronous and held is not None:
                    held.identify_stragglers()
                t2 = time.perf_counter_ns()
                held = rep
                Detector.rings.lib.nvrx_report_clocks(clk)
                if lane is not None and Detector._lane is lane and len(t_harvest) == n_h:
                    # served by the steady-state lane (one C call): the wait for the window's kernel records is its first stage
                    Detector.rings.lib.nvrx_window_clocks(wclk)
                    t_harvest.append((wclk[1] - wclk[0]) * 1e3)
                    lanes += i >= 2
                if i >= 2:
                    t.append(t1 - t0)
                    t_late.append(t2 - t1)
                    stages.append([tg - t0, t1 - tg, (clk[1] - clk[0]) * 1e3, (clk[2] - clk[1]) * 1e3, (clk[3] - clk[2]) * 1e3,
                                   (clk[5] - clk[3]) * 1e3, (clk[6] - clk[5]) * 1e3 if not asynchronous else 0.0,
                                   (clk[6] - clk[0]) * 1e3 if not asynchronous else (clk[5] - clk[0]) * 1e3])
            a = np.asarray(t, dtype=np.float64) / 1e3
            res = {"us_median": round(float(np.median(a)), 2), "us_p95": round(float(np.percentile(a, 95)), 2),
                   "us_max": round(float(a.max()), 2), "reports": len(t),
                   "of_which_harvest_us_median": round(float(np.median(t_harvest[2:])) / 1e3, 2),
                   "kernel_keys": len(Detector.rings.kernel_row_names), "reports_served_by_the_lane": int(lanes)}
            st_ = np.median(np.asarray(stages, dtype=np.float64), axis=0) / 1e3
            res["stages_us_median"] = dict(zip(("generate_report", "identify_stragglers", "c_stream_ordering", "c_flush_scatter",
                                                "c_row_stats_launch", "c_score_launch", "c_wait_completion", "c_call_total"),
                                               (round(float(v), 2) for v in st_)))
            if asynchronous:
                res["read_one_interval_later_us_median"] = round(float(np.median(t_late)) / 1e3, 2)
            return res
        finally:
            Detector.shutdown()

    try:
        out["report_at_cadence_kernels"] = {
            "synchronous": cadence(False, 4), "asynchronous": cadence(True, 4),
            "workload": "the transformer step above in a GPU-timed section, 40 steps between reports, tens of thousands of traced dispatches per "
                        "window appended to their rings by the tracer's thread as they complete; each generate_report() timed alone "
                        "after the step's device synchronisation (synchronous: call -> identify_stragglers() returned)"}
    except Exception as e:  # noqa: BLE001
        out["report_at_cadence_kernels"] = {"error": f"{type(e).__name__}: {str(e)[-300:]}"}
    out["gpu_timing_mode"] = ktrace.timing_mode()
    out["registered_through"] = ktrace._setup_route
    print("KERNELS_MODE " + json.dumps(out), flush=True)


def _kernels_mode_leg(child: str = "kernels_mode", timeout_s: float = 420.0):
    """Run ``_kernels_mode_child`` in a fresh interpreter on the same GPU (this process is idle meanwhile)."""
    import subprocess

    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "NVRX_GPU_TIMING"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", child], capture_output=True, text=True,
                       timeout=timeout_s, env=env)
    lines = [l for l in p.stdout.splitlines() if l.startswith("KERNELS_MODE ")]
    if p.returncode != 0 or not lines:
        return {"error": f"child exited {p.returncode}: {(p.stderr or p.stdout)[-400:]}"}
    return json.loads(lines[-1][len("KERNELS_MODE "):])


def _kernel_source_sha() -> str:
    """sha256 (16 hex digits) of the text of ``k_row_stats`` -- everything between its header comment and the next kernel's
    -- in csrc/nvrx_straggler.hip: the traffic figure belongs to that kernel, host-side edits of the file do not touch it."""
    import hashlib

    with open(os.path.join(REPO, "nvidia-resiliency-ext_amd", "csrc", "nvrx_straggler.hip"), "rb") as f:
        text = f.read()
    a, b = text.find(b"// k_row_stats: one workgroup per timing row."), text.find(b"// k_scatter:")
    return hashlib.sha256(text[a:b] if 0 <= a < b else text).hexdigest()[:16]


def _pmc_traffic(rows: int):
    """HBM bytes per k_row_stats launch from the rocprofv3 PMC pass of tools/archive/run_gpu_round.sh (separate run, --pmc
    FETCH_SIZE with --kernel-trace only; FETCH_SIZE doubled per MI355X_MICROARCH.md section HBM).  The summary
    records the sha of the kernel source it was measured on: a summary of any other source is stale and reported as
    null rather than quoted."""
    path = os.path.join(REPO, "profiles", "pmc_row_stats.json")
    try:
        with open(path) as f:
            d = json.load(f)
        if d.get("kernel_source_sha16") != _kernel_source_sha():
            return None
        return d.get("rows", {}).get(str(rows), {}).get("hbm_bytes_per_launch")
    except Exception:
        return None


def _pmc_traffic_of_an_older_source(rows: int):
    """When ``traffic`` is null because the kernel's text changed after the last PMC pass: that pass' figure, labelled
    with the sha it belongs to -- information, not this source's measurement."""
    try:
        with open(os.path.join(REPO, "profiles", "pmc_row_stats.json")) as f:
            d = json.load(f)
        if d.get("kernel_source_sha16") == _kernel_source_sha():
            return None
        b = d.get("rows", {}).get(str(rows), {}).get("hbm_bytes_per_launch")
        return None if b is None else {"hbm_bytes_per_launch": b, "kernel_source_sha16": d.get("kernel_source_sha16"),
                                       "source": d.get("source"), "this_source_sha16": _kernel_source_sha()}
    except Exception:
        return None


def _kernel_leg(job, steps, samples, cold=False, sweep=None):
    """Average k_row_stats duration over `steps` reports of `job` (hipExtLaunchKernel start/stop events on the launch
    stream).  cold=True: a 1 GiB sweep between reports evicts L2 and the Infinity Cache, so the rows come from HBM."""
    job.rings.timing_enable(True)
    job.rings.timing_read(reset=True)
    for _ in range(steps):
        if cold:
            sweep.add_(1.0)
            torch.cuda.synchronize()
        job.rearm(samples)
        job.report()
    torch.cuda.synchronize()
    total_us, launches = job.rings.timing_read(reset=True)
    job.rings.timing_enable(False)
    return total_us / max(launches, 1), launches


def _roof(kern_us, alg_bytes):
    achieved = alg_bytes / (kern_us * 1e-6) / 1e9 if kern_us > 0 else 0.0
    return {"kernel_us_avg": round(kern_us, 3), "achieved": round(achieved, 1), "frac": round(achieved / HBM_PEAK_GBS, 4)}


def _n8_shape_leg(steps, warmup):
    """The per-GPU work of the 8-GPU production shape on this GPU: ONE logical rank, 64 rows x 10 000 samples (2.56 MB).
    Report latency without an exchange + the statistics kernel against the roofline at that shape."""
    import synth
    from nvrx_straggler import ktrace as _ktrace
    from nvrx_straggler.folded import FoldedJob

    job = FoldedJob(total_ranks=1, section_names=[synth.section_name(s) for s in range(SECTIONS)], ring_cap=SAMPLES,
                    node_name="node0")
    try:
        job.load(0, synth.stress_samples(0, SECTIONS, SAMPLES))
        gc.collect()  # before the warm-up, never between it and the timed region (see main)
        for _ in range(warmup):
            job.rearm(SAMPLES)
            job.report().identify_stragglers()
        torch.cuda.synchronize()
        t = []
        for _ in range(steps):
            t0 = time.perf_counter_ns()
            job.rearm(SAMPLES)
            job.report().identify_stragglers()  # held and read, as in the headline loop
            t.append(time.perf_counter_ns() - t0)
        torch.cuda.synchronize()
        us = float(np.mean(t)) / 1e3
        kern_us, launches = _kernel_leg(job, steps, SAMPLES)
        alg = SECTIONS * SAMPLES * 4
        out = {"workload": f"1 rank x {SECTIONS} sections x {SAMPLES} samples (what ONE GPU holds at 8 GPUs), no exchange",
               "report_us": round(us, 2), "report_us_median": round(float(np.median(t)) / 1e3, 2), "bound": "hbm", "kernel": "k_row_stats", "peak": HBM_PEAK_GBS, "unit": "GB/s",
               "algorithmic_bytes_per_launch": alg, "launches_timed": launches, "traffic": _pmc_traffic(SECTIONS)}
        out.update(_roof(kern_us, alg))
        return out
    finally:
        job.close()


def _detector_leg(steps, warmup):
    """Detector-level latency: the real ``Detector.generate_report()`` (harvest of GPU regions, occupancy check,
    report, ring reset -- straggler.py:228-244) over one rank's 64 resident sections x 10 000 samples."""
    import synth
    from nvrx_straggler import Detector
    from nvrx_straggler.straggler import CustomSection

    old_cap = CustomSection.max_elapseds_len
    CustomSection.max_elapseds_len = SAMPLES
    Detector.initialize(scores_to_compute="all", gather_on_rank0=True, node_name="node0")
    try:
        x = torch.from_numpy(synth.stress_samples(0, SECTIONS, SAMPLES)).cuda()
        for s in range(SECTIONS):
            with Detector.detection_section(synth.section_name(s), profile_cuda=False):
                pass
        Detector._reset_sections_elapseds()
        rings = Detector.rings
        for s in range(SECTIONS):
            rings.push_device(Detector.custom_sections[synth.section_name(s)].row, x[s].contiguous())
        torch.cuda.synchronize()
        rings.backend.synchronize()

        def step():
            for row in range(rings.rows_used):
                rings.set_count(row, SAMPLES)
            return Detector.generate_report().identify_stragglers()

        for _ in range(warmup):
            step()
        t = []
        for _ in range(steps):
            for row in range(rings.rows_used):
                rings.set_count(row, SAMPLES)
            t0 = time.perf_counter()
            Detector.generate_report().identify_stragglers()
            t.append(time.perf_counter() - t0)
        return {"us_median": round(float(np.median(t)) * 1e6, 2), "us_p95": round(float(np.percentile(t, 95)) * 1e6, 2),
                "workload": f"Detector.generate_report() + identify_stragglers() incl. harvest / occupancy check / ring reset, 1 rank x {SECTIONS} "
                            f"sections x {SAMPLES} resident samples, relative+individual scores"}
    finally:
        Detector.shutdown()
        CustomSection.max_elapseds_len = old_cap


def _section_entry_leg(entries: int = 3000):
    """Host cost of ONE ``Detector.detection_section`` entry (enter + exit, empty body), the figure BASELINE.md section 3
    quotes for the reference at ~2.7 us (straggler.py:287-348: perf_counter_ns pair, deque append, CUPTI refcount):
    ``profile_cuda=False`` (one staged host sample) and ``profile_cuda=True`` (two one-thread stamp kernels on the
    caller's stream; their cost to that STREAM is in profiles/r04e_stamp_cost.txt: +3.5 us per entry behind a busy
    kernel, against +7.9 us for a hipEventRecord pair)."""
    from nvrx_straggler import Detector

    Detector.initialize(scores_to_compute=["individual_perf_scores"], gather_on_rank0=False, node_name="node0")
    try:
        out = {}
        for label, gpu in (("profile_cuda_false_us", False), ("profile_cuda_true_us", True)):
            name = "entry_" + label
            for _ in range(200):
                with Detector.detection_section(name, profile_cuda=gpu):
                    pass
            torch.cuda.synchronize()
            t = []
            for _ in range(entries):
                t0 = time.perf_counter_ns()
                with Detector.detection_section(name, profile_cuda=gpu):
                    pass
                t.append(time.perf_counter_ns() - t0)
                if gpu and len(t) % 256 == 0:
                    torch.cuda.synchronize()  # keep the queue of stamp kernels short: this is the host's cost per entry
            torch.cuda.synchronize()
            out[label] = round(float(np.median(t)) / 1e3, 2)
            out[label.replace("_us", "_p95_us")] = round(float(np.percentile(t, 95)) / 1e3, 2)
            Detector.generate_report()
        # NOT measured by this run: figures of earlier profile runs, kept apart so that nobody takes them for this box's
        out["quoted_from_profiles"] = {
            "reference_python_us": {"value": 2.7, "source": "BASELINE.md section 3 (survey probe of the reference's Python path, build container)"},
            "stream_us_per_gpu_timed_entry": {"value": 3.5, "source": "profiles/r04e_stamp_cost.txt (tools/archive/micro/stamp_cost.cpp, round 4, "
                                              "NVRX_STAMP_ARGFREE=1): what the two stamp kernels add to a busy user stream; a hipEventRecord pair: 7.9"}}
        out["note"] = ("host time of one detection_section entry with an empty body, median of %d; "
                       "profile_cuda_true_event_mode_us = the same entry with NVRX_GPU_TIMING=event (a hipEventRecord pair)" % entries)
    finally:
        Detector.shutdown()
    # the same entry timed by a hipEvent pair (NVRX_GPU_TIMING=event is read when the Detector's profiler is built)
    saved = os.environ.get("NVRX_GPU_TIMING")
    os.environ["NVRX_GPU_TIMING"] = "event"
    try:
        Detector.initialize(scores_to_compute=["individual_perf_scores"], gather_on_rank0=False, node_name="node0")
        try:
            for _ in range(200):
                with Detector.detection_section("entry_event", profile_cuda=True):
                    pass
            torch.cuda.synchronize()
            Detector.generate_report()
            t = []
            for i in range(min(entries, 2000)):
                t0 = time.perf_counter_ns()
                with Detector.detection_section("entry_event", profile_cuda=True):
                    pass
                t.append(time.perf_counter_ns() - t0)
                if len(t) % 256 == 0:
                    torch.cuda.synchronize()
                    Detector.generate_report()      # (harvests the event pairs: the pool is finite)
            out["profile_cuda_true_event_mode_us"] = round(float(np.median(t)) / 1e3, 2)
        finally:
            Detector.shutdown()
    except Exception as e:  # noqa: BLE001  (an extra figure: its failure must not take the leg down)
        out["profile_cuda_true_event_mode_us"] = f"{type(e).__name__}: {str(e)[-200:]}"
    finally:
        if saved is None:
            os.environ.pop("NVRX_GPU_TIMING", None)
        else:
            os.environ["NVRX_GPU_TIMING"] = saved
    return out


def _side_leg(fn, *a, **k):
    """A side leg must never take the headline line down with it: its failure becomes its value."""
    try:
        return fn(*a, **k)
    except Exception as e:  # noqa: BLE001
        return {"error": f"{type(e).__name__}: {str(e)[-300:]}"}


def _route_leg(route: str, world: int, rank: int, steps: int, warmup: int):
    """The headline loop once more on ONE named exchange route (N > 1): a fresh job (its own rings, generator and -- for the
    in-stream routes -- communicator / windows), ``warmup`` + ``steps`` reports, each step's time; then the route's floor.
    Collective: every rank runs it.  What the route's checked trial said is in ``selection``; a route the trial dropped is
    reported as dropped (the reports then ran on torch.distributed, and the figure says so)."""
    import synth
    from nvrx_straggler.folded import FoldedJob

    saved = os.environ.get("NVRX_EXCHANGE")
    os.environ["NVRX_EXCHANGE"] = route
    job = None
    try:
        job = FoldedJob(total_ranks=TOTAL_RANKS, section_names=[synth.section_name(s) for s in range(SECTIONS)],
                        ring_cap=SAMPLES, node_name=f"node{rank}")
        for lr, r in enumerate(job.logical_ranks()):
            job.load(lr, synth.stress_samples(r, SECTIONS, SAMPLES, slow_rank=3, slow_factor=1.5))
        torch.cuda.synchronize()
        found = None
        for _ in range(warmup + 3):
            job.rearm(SAMPLES)
            rep = job.report()
            found = rep.identify_stragglers() if rep is not None else None
        torch.cuda.synchronize()
        dist.barrier()
        t = []
        for _ in range(steps):
            t0 = time.perf_counter_ns()
            job.rearm(SAMPLES)
            rep = job.report()
            found = rep.identify_stragglers() if rep is not None else None
            t.append(time.perf_counter_ns() - t0)
        torch.cuda.synchronize()
        ok = True
        if rank == 0:
            flagged = found["straggler_sections_relative"]
            ok = len(flagged) == SECTIONS and all({s.rank for s in v} == {3} for v in flagged.values())
        info = dict(job.reporter.exchange_info)
        direct = job.reporter._direct
        took = "in-stream" if direct is not None else "torch.distributed"
        dropped = [k for k in ("rccl_rejected", "peer_rejected") if info.get(k)]
        med = torch.tensor([float(np.median(t)) / 1e3], dtype=torch.float64, device="cuda")
        dist.all_reduce(med, op=dist.ReduceOp.MAX)
        out = {"us_median": round(float(med.item()), 2), "steps": steps, "flagged_set_right": bool(ok),
               "ran_on": getattr(direct, "route", None) or info.get("route", took),
               "status": "ok" if (route == "c10d" or direct is not None) else "dropped: " + (", ".join(dropped) or "the route could not be built on this group")
               + " -- the reports ran on torch.distributed", "selection": info}
        ranks_fn = getattr(direct, "comm_ranks", None)
        if ranks_fn is not None:
            out["ncclCommCount"] = ranks_fn()
        # the route's floor on this machine: ONE rank's production row (129 f32) all-gathered on the same communicator / stream
        from nvrx_straggler import dist_utils as _du

        L1 = 2 * SECTIONS + 1
        f_send = torch.zeros(L1, dtype=torch.float32, device="cuda")
        f_recv = torch.zeros(world * L1, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        be_ = job.backend

        def floor_once():
            if direct is not None and hasattr(direct, "all_gather"):
                direct.all_gather(f_send.data_ptr(), f_recv.data_ptr(), L1, be_.stream_handle)
            else:
                with be_.stream_context():
                    _du.all_gather_rows(f_send.view(1, L1), f_recv.view(world, L1), job.reporter.group)
            be_.synchronize()

        for _ in range(5):
            floor_once()
        t_fl = []
        for _ in range(50):
            t0 = time.perf_counter()
            floor_once()
            t_fl.append(time.perf_counter() - t0)
        fl = torch.tensor([float(np.median(t_fl)) * 1e6], dtype=torch.float64, device="cuda")
        dist.all_reduce(fl, op=dist.ReduceOp.MAX)
        out["floor_us"] = round(float(fl.item()), 2)
        return out
    finally:
        if job is not None:
            try:
                job.close()
            except Exception:  # noqa: BLE001
                pass
        if saved is None:
            os.environ.pop("NVRX_EXCHANGE", None)
        else:
            os.environ["NVRX_EXCHANGE"] = saved


def _routes_table(world: int, rank: int, steps: int, warmup: int, headline_route: str, per_route_timeout_s: float, emit):
    """N > 1: the same reports on every OTHER exchange route, so that one run of the driver's scaling bench yields the whole
    table (c10d = the default, rccl = ncclAllGather on a second communicator in the detector's stream, peer = xGMI peer
    stores into IPC windows).  The legs run on the MAIN thread, like the headline (on a helper thread the same torch.distributed
    route measured 1.5-17 x slower than the headline with gloo ranks sharing one GPU, profiles/r06n: not a fair table), under a
    watchdog: none of the in-stream routes has ever run across two real devices, and a route that does not come back must
    cost its own entry, not the line -- when a leg's deadline passes the watchdog calls ``emit(table)`` (rank 0 prints the
    line it has, with the routes seen so far) and the process leaves through os._exit.  ``emit`` prints at most once.
    Returns (table, clean): ``clean`` False after an error in a leg -- the ranks may then disagree about where they are, so
    nothing collective may follow."""
    import threading

    table, clean = {}, True
    for route in ("c10d", "rccl", "peer"):
        if route == headline_route:
            continue
        if not clean:
            table[route] = {"status": "not run: an earlier route failed"}
            continue

        def bail(route=route):
            table[route] = {"status": f"timed out after {per_route_timeout_s:.0f} s"}
            for later in ("c10d", "rccl", "peer"):
                if later != headline_route and later not in table:
                    table[later] = {"status": "not run: an earlier route did not come back"}
            emit(table)
            sys.stdout.flush()
            sys.stderr.flush()
            os._exit(0)

        timer = threading.Timer(per_route_timeout_s, bail)
        timer.daemon = True
        timer.start()
        try:
            # (test hooks of tests/test_gpu_bench_contract.py: what the line looks like when a leg dies or never comes back)
            if os.environ.get("NVRX_BENCH_TEST_DIE_IN_ROUTE") == route and rank == 0:
                import signal

                os.kill(os.getpid(), signal.SIGSEGV)
            if os.environ.get("NVRX_BENCH_TEST_HANG_IN_ROUTE") == route:
                time.sleep(10 * per_route_timeout_s)
            table[route] = _route_leg(route, world, rank, steps, warmup)
        except BaseException as e:  # noqa: BLE001
            table[route] = {"status": f"error: {type(e).__name__}: {str(e)[-300:]}"}
            clean = False  # (a rank that raised has left the others inside a collective; their watchdogs end them)
        finally:
            timer.cancel()
    return table, clean


def _dump_outputs(out_dir: str, rep, found, section_names, total_ranks: int = TOTAL_RANKS) -> list:
    """``--dump-outputs DIR``: what a caller of the timed step holds after the last one -- the Report's score mappings and its
    local section statistics (float64, the exact values of the f32 results) and the flagged sets identify_stragglers()
    returned (float32 0/1 tables) -- as DIR/<name>.npy, rows in section order, columns in rank order.  A GPU score mapping is
    written only when it holds a finite score: the benchmark's job times no GPU work, so both are NaN for every rank by
    construction and carry no result (their flagged sets, always empty then, are written).  A few KB in all; the inputs are
    seeded (synth.stress_samples), so two builds can be compared file by file."""
    from nvrx_straggler import Statistic

    os.makedirs(out_dir, exist_ok=True)
    ranks = range(total_ranks)
    arrays = {}
    for field in ("gpu_relative_perf_scores", "gpu_individual_perf_scores"):
        m = getattr(rep, field)
        scores = np.array([m.get(r, np.nan) for r in ranks], dtype=np.float64)
        if np.isfinite(scores).any():
            arrays[field] = scores
    for field in ("section_relative_perf_scores", "section_individual_perf_scores"):
        m = getattr(rep, field)
        arrays[field] = np.array([[m.get(n, {}).get(r, np.nan) for r in ranks] for n in section_names], dtype=np.float64)
    summ = rep.local_section_summaries
    arrays["local_section_summaries"] = np.array([[summ[n][s] if n in summ else np.nan for s in Statistic] for n in section_names],
                                                 dtype=np.float64)
    for key in ("straggler_gpus_relative", "straggler_gpus_individual"):
        flagged = {s.rank for s in found[key]}
        arrays[key] = np.array([r in flagged for r in ranks], dtype=np.float32)
    for key in ("straggler_sections_relative", "straggler_sections_individual"):
        flagged = {n: {s.rank for s in v} for n, v in found[key].items()}
        arrays[key] = np.array([[r in flagged.get(n, ()) for r in ranks] for n in section_names], dtype=np.float32)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return sorted(arrays)


_SIDECAR_SRC = r"""
import sys, signal
for s in (signal.SIGTERM, signal.SIGINT, signal.SIGHUP):
    signal.signal(s, signal.SIG_IGN)
line = sys.stdin.buffer.readline()
word = sys.stdin.buffer.readline()
if word.strip() != b"DONE":
    sys.stdout.buffer.write(line)
    sys.stdout.buffer.flush()
"""


def _headline_sidecar(out: dict, headline_mode: str):
    """A tiny interpreter (no torch, its own session) that is handed the finished line with every other route marked
    "process died", and prints it only if this process goes away without saying DONE."""
    import subprocess

    fallback = dict(out)
    died = {"status": "not known: rank 0's process died during the route legs (a signal inside an untested route); the headline above was complete"}
    fallback["routes"] = {headline_mode: {"us_median": out.get("us_per_report_median"), "status": "ok (the headline of this line)"},
                          **{r: dict(died) for r in ("c10d", "rccl", "peer") if r != headline_mode}}
    try:
        p = subprocess.Popen([sys.executable, "-S", "-E", "-c", _SIDECAR_SRC], stdin=subprocess.PIPE, start_new_session=True, close_fds=True)
        p.stdin.write(json.dumps(fallback).encode() + b"\n")
        p.stdin.flush()
        return p
    except Exception:  # noqa: BLE001
        return None


def _self_launch(n: int) -> int:
    """``python bench.py --gpus N`` without a launcher: start N copies of this command, one rank each, with the
    environment torch.distributed.run would give them (rendezvous on 127.0.0.1, a free port).  Rank 0 prints the JSON
    line; the first failing rank ends the run (its exact PIDs are killed, nothing is matched by pattern)."""
    import socket
    import subprocess

    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), NVRX_BENCH_SELF_LAUNCHED="1")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rc = 0
    deadline = time.time() + float(os.environ.get("NVRX_BENCH_TIMEOUT_S", "1500"))
    live = list(procs)
    while live:
        for p in list(live):
            code = p.poll()
            if code is None:
                continue
            live.remove(p)
            if code != 0 and rc == 0:
                rc = code
        if rc != 0 or time.time() > deadline:
            for p in live:
                p.kill()
            for p in live:
                p.wait()
            return rc or 124
        time.sleep(0.05)
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--full", action="store_true", help="also run every leg besides the headline (roofline, report read, exchange "
                    "and routes, cold / N=8-shape / Detector legs, host inputs, cadence, per-kernel mode, per-step overhead, CPU "
                    "baseline); the --no-* options below pick among them")
    ap.add_argument("--dump-outputs", metavar="DIR", default="", help="write what the last timed step returned as DIR/<name>.npy")
    ap.add_argument("--cpu-reps", type=int, default=60)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--backend", default="nccl", help="process-group backend for N > 1 (nccl = RCCL; gloo lets the N > 1 flow "
                    "be exercised with several ranks sharing one GPU)")
    ap.add_argument("--no-overhead", action="store_true", help="skip the per-step overhead leg (config #4)")
    ap.add_argument("--no-host-inputs", action="store_true", help="skip the PCIe-inclusive leg (samples handed over from host memory)")
    ap.add_argument("--no-extra-legs", action="store_true", help="skip the N=8-shape, cold-cache and Detector-level legs")
    ap.add_argument("--overhead-steps", type=int, default=100)
    ap.add_argument("--overhead-blocks", type=int, default=6)
    ap.add_argument("--no-cadence", action="store_true", help="skip the production-cadence leg (one report per 100 training steps)")
    ap.add_argument("--cadence-reports", type=int, default=30)
    ap.add_argument("--dump-steps", action="store_true", help="add the per-step latencies of the timed region to the JSON line")
    ap.add_argument("--no-kernels-mode", action="store_true", help="skip the per-kernel-tracing legs (they run in a child interpreter)")
    ap.add_argument("--no-routes", action="store_true", help="N > 1: skip the legs that repeat the timed loop on the other exchange routes")
    ap.add_argument("--route-timeout", type=float, default=90.0, help="N > 1: seconds one exchange route's leg may take")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child in ("kernels_mode", "stamp_mode"):
        return _kernels_mode_child(args.child.split("_")[0])
    if args.steps < 1:
        raise SystemExit("--steps must be at least 1")

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        if TOTAL_RANKS % args.gpus:
            raise SystemExit(f"--gpus must divide {TOTAL_RANKS}")
        if args.backend == "nccl" and torch.cuda.device_count() < args.gpus:
            raise SystemExit(f"--gpus {args.gpus} with RCCL needs {args.gpus} visible GPUs, found {torch.cuda.device_count()} "
                             "(RCCL refuses two ranks on one device; --backend gloo lets ranks share a GPU)")
        raise SystemExit(_self_launch(args.gpus))

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if TOTAL_RANKS % world:
        raise SystemExit(f"--gpus must divide {TOTAL_RANKS}")
    device_index = local_rank % max(torch.cuda.device_count(), 1)  # == local_rank on a node with one GPU per rank
    torch.cuda.set_device(device_index)
    if world > 1:
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", device_index))
        else:
            dist.init_process_group(args.backend)

    # which physical devices the ranks really run on: with --backend gloo several ranks may share one, and the line must
    # not call that "N GPUs"
    props = torch.cuda.get_device_properties(device_index)
    ident = (os.uname().nodename, getattr(props, "pci_domain_id", -1), getattr(props, "pci_bus_id", -1),
             getattr(props, "pci_device_id", device_index), str(getattr(props, "uuid", "")))
    if world > 1:
        idents = [None] * world
        dist.all_gather_object(idents, ident)
    else:
        idents = [ident]
    distinct_devices = len(set(idents))

    import synth
    from nvrx_straggler import ktrace as _ktrace
    from nvrx_straggler.folded import FoldedJob

    job = FoldedJob(total_ranks=TOTAL_RANKS, section_names=[synth.section_name(s) for s in range(SECTIONS)],
                    ring_cap=SAMPLES, node_name=f"node{rank}")
    for lr, r in enumerate(job.logical_ranks()):
        job.load(lr, synth.stress_samples(r, SECTIONS, SAMPLES, slow_rank=3, slow_factor=1.5))
    torch.cuda.synchronize()

    call_ns = []

    def step():
        # the report is held and its flagged-straggler set read (rank 0 under gather_on_rank0; the others get None):
        # identify_stragglers() waits for / copies the scores and flags out of the result block
        t_in = time.perf_counter_ns()
        job.rearm(SAMPLES)
        rep = job.report()
        call_ns.append(time.perf_counter_ns() - t_in)  # re-arm + the call alone: what round 2's loop timed
        return rep, (rep.identify_stragglers() if rep is not None else None)

    def sync_all():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    def check_flagged(found):
        # correctness guard inside the bench: flagged set of the x1.5 rank at the default threshold
        flagged = found["straggler_sections_relative"]
        assert len(flagged) == SECTIONS and all({s.rank for s in v} == {3} for v in flagged.values()), "wrong flagged set"

    # One full collection BEFORE the warm-up, and what survives it is moved out of the collector's sight: a generation-2
    # pass of Python's cyclic collector (45-70 ms with torch imported) otherwise lands inside some leg by accident of
    # allocation counts and reads as +200 us per report.  It must not sit between the warm-up and the timed region: the
    # collection walks every object of the process and leaves the host's caches cold, and the first report after it
    # took 85-110 us + 50 us for the read instead of 25 + 9 (tools/archive/outlier_probe.py, profiles/r03a_outlier_probe.txt) --
    # that was the one ~175 us step of r02's 20-step driver run.  The collector stays enabled.
    gc.collect()
    gc.freeze()
    # correctness guard (not timed, not part of the warm-up count): 25 reports, the flagged set of EVERY one checked
    rep = found = None
    for _ in range(25):
        rep, found = step()
        if rank == 0:
            check_flagged(found)
    for _ in range(args.warmup):
        rep, found = step()
    sync_all()
    per_step = []
    del call_ns[:]
    t0 = time.perf_counter()
    for _ in range(args.steps):
        ts = time.perf_counter_ns()
        rep, found = step()
        per_step.append(time.perf_counter_ns() - ts)
    t_loop = time.perf_counter()
    sync_all()
    elapsed = time.perf_counter() - t0
    closing_sync_us = (time.perf_counter() - t_loop) * 1e6
    call_us_median = float(np.median(call_ns[: args.steps])) / 1e3
    if rank == 0:
        check_flagged(found)  # the last timed report
        if args.dump_outputs:
            _dump_outputs(args.dump_outputs, rep, found, job.section_names)

    # what READING the rest of a report costs on the host (rank 0): the six dict mappings, built on first access
    report_read = None
    if args.full and rank == 0:
        t_ident, t_maps = [], []
        for _ in range(min(args.steps, 50)):
            job.rearm(SAMPLES)
            r = job.report()
            ta = time.perf_counter_ns()
            r.identify_stragglers()
            tb = time.perf_counter_ns()
            for f in ("gpu_relative_perf_scores", "section_relative_perf_scores", "gpu_individual_perf_scores",
                      "section_individual_perf_scores", "local_section_summaries", "local_kernel_summaries"):
                getattr(r, f)
            tc = time.perf_counter_ns()
            t_ident.append(tb - ta)
            t_maps.append(tc - tb)
        # the same while the caller still HOLDS the previous report: nothing can be recycled, every dict is built anew
        t_held, held = [], None
        for _ in range(min(args.steps, 30)):
            job.rearm(SAMPLES)
            r2 = job.report()
            r2.identify_stragglers()
            tb = time.perf_counter_ns()
            for f in ("gpu_relative_perf_scores", "section_relative_perf_scores", "gpu_individual_perf_scores",
                      "section_individual_perf_scores", "local_section_summaries", "local_kernel_summaries"):
                getattr(r2, f)
            t_held.append(time.perf_counter_ns() - tb)
            held = r2  # noqa: F841  (kept alive across the next iteration on purpose)
        del held, r2
        report_read = {"identify_stragglers_us": round(float(np.median(t_ident)) / 1e3, 2),
                       "all_six_mappings_us": round(float(np.median(t_maps)) / 1e3, 2),
                       "all_six_mappings_previous_report_held_us": round(float(np.median(t_held)) / 1e3, 2),
                       "note": "host cost of reading one report: identify_stragglers() at the default thresholds (flag bytes "
                               "of the score kernel; part of `value`) and building the six dict mappings "
                               f"({TOTAL_RANKS} ranks x {SECTIONS} sections of scores x 2 families, {SECTIONS} x 6 local "
                               "statistics; not part of `value`).  all_six_mappings_us: the caller has dropped the previous "
                               "report, as a training loop does -- its dicts are refilled in place (nvrx_pyread.c, recycling); "
                               "..._previous_report_held_us: it still holds it, every dict is built anew"}
    elif args.full and world > 1:
        for _ in range(min(args.steps, 50) + min(args.steps, 30)):  # collective: the other ranks take part in rank 0's reports (both loops)
            job.rearm(SAMPLES)
            job.report()

    # instrumented pass: hipEvent pair around every statistics-kernel launch, on its launch stream
    elapsed_instr = 0.0
    score_wait, score_tail, score_staged = [], [], []
    if args.full:
        job.rings.timing_enable(True)
        sync_all()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            step()
            plan = job.reporter._ring_plan
            if plan is not None:  # the score kernel's own clocks (10 ns ticks of the constant-rate wall clock), see nvrx_score
                score_wait.append(int(plan.ws.meta[6]))
                score_tail.append(int(plan.ws.meta[7]) & 0xFFFF)
                score_staged.append(int(plan.ws.meta[7]) >> 16)
        sync_all()
        elapsed_instr = time.perf_counter() - t1
        kern_total_us, kern_launches = job.rings.timing_read(reset=True)
        job.rings.timing_enable(False)

    # the report's one collective on its own (N > 1): enqueue on the detector's stream, wait for that stream
    exchange = None
    if args.full and world > 1:
        try:
            ws = job.reporter._ring_plan.ws
            for _ in range(10):
                job.reporter._exchange(job.backend, ws)
            job.backend.synchronize()
            t_ex = []
            for _ in range(100):
                t0 = time.perf_counter()
                job.reporter._exchange(job.backend, ws)
                job.backend.synchronize()
                t_ex.append(time.perf_counter() - t0)
            # the floor of that collective on this machine: ONE rank's row -- 129 floats = 516 B, the production payload of a
            # one-rank-per-GPU job -- all-gathered on the SAME communicator and stream, nothing else enqueued
            L1 = 2 * SECTIONS + 1
            f_send = torch.zeros(L1, dtype=torch.float32, device="cuda")
            f_recv = torch.zeros(world * L1, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            direct = job.reporter._direct
            be_ = job.backend
            from nvrx_straggler import dist_utils as _du

            def floor_once():
                if direct is not None and hasattr(direct, "all_gather"):
                    direct.all_gather(f_send.data_ptr(), f_recv.data_ptr(), L1, be_.stream_handle)
                else:
                    with be_.stream_context():  # (RCCL group: all_gather_into_tensor; gloo: the host hop the reports take too)
                        _du.all_gather_rows(f_send.view(1, L1), f_recv.view(world, L1), job.reporter.group)
                be_.synchronize()

            for _ in range(10):
                floor_once()
            t_fl = []
            for _ in range(100):
                t0 = time.perf_counter()
                floor_once()
                t_fl.append(time.perf_counter() - t0)
            floor_us = float(np.median(t_fl)) * 1e6
            exchange = {"us_median": float(np.median(t_ex)) * 1e6,
                        "floor_us": round(floor_us, 2),
                        "floor_note": f"bare all-gather of {L1} f32 ({L1 * 4} B) per rank on the same communicator / stream + stream wait",
                        # ring all-gather: every rank forwards (world - 1) rows over one xGMI link (~153 GB/s per link, MI355X_MICROARCH.md)
                        "xgmi": {"bytes_per_link": int((world - 1) * ws.local_ranks * ws.L * 4), "peak_gbs_per_link": 153.0,
                                 "achieved_gbs": round((world - 1) * ws.local_ranks * ws.L * 4 / (float(np.median(t_ex)) * 1e9) if t_ex else 0.0, 6),
                                 "frac": round((world - 1) * ws.local_ranks * ws.L * 4 / (float(np.median(t_ex)) * 1e9) / 153.0, 8),
                                 "note": "latency-bound by construction: half a kilobyte per rank; the fraction of the link's bandwidth is "
                                         "reported because north_star asks for it, the figure to watch is us_median against floor_us"},
                        "route": getattr(job.reporter._direct, "route", None) or job.reporter.exchange_info.get("route", "torch.distributed"),
                        "selection": dict(job.reporter.exchange_info),
                        "bytes_per_rank": int(ws.local_ranks * ws.L * 4),
                        "ranks": world, "distinct_devices": distinct_devices}
        except Exception as e:  # noqa: BLE001  (deterministic on every rank: same state everywhere)
            exchange = {"error": str(e)[-200:]}

    # the max over ranks of the timed regions is taken NOW, while every rank is certainly still in step
    if world > 1:
        _t = torch.tensor([elapsed, elapsed_instr, exchange.get("us_median", 0.0) if exchange and "us_median" in exchange else 0.0],
                          dtype=torch.float64, device="cuda")
        dist.all_reduce(_t, op=dist.ReduceOp.MAX)
        times_max = _t.tolist()

    # the same kernel with its rows coming from HBM: a 1 GiB sweep between reports evicts L2 and the Infinity Cache
    cold = None
    n8 = None
    detector_leg = section_entry = None
    if args.full and world == 1 and not args.no_extra_legs:
        sweep = torch.zeros(1 << 28, dtype=torch.float32, device="cuda")
        cold_us, cold_n = _kernel_leg(job, min(args.steps, 30), SAMPLES, cold=True, sweep=sweep)
        del sweep
        cold = _roof(cold_us, job.local_ranks * SECTIONS * SAMPLES * 4)
        cold["launches_timed"] = cold_n
        cold["note"] = "1 GiB device sweep between reports: rows fetched from HBM, not from L2 / Infinity Cache"
        n8 = _side_leg(_n8_shape_leg, args.steps, args.warmup)
        detector_leg = _side_leg(_detector_leg, args.steps, args.warmup)
        section_entry = _side_leg(_section_entry_leg)

    host_inputs = None
    if args.full and world == 1 and not args.no_host_inputs:
        try:
            host = [synth.stress_samples(r, SECTIONS, SAMPLES, slow_rank=3, slow_factor=1.5) for r in job.logical_ranks()]
            t_host = []
            for _ in range(6):
                job.rings.reset()
                sync_all()
                t0 = time.perf_counter()
                for lr in range(job.local_ranks):
                    job.load(lr, host[lr])
                job.report()
                t_host.append(time.perf_counter() - t0)
            nbytes = job.local_ranks * SECTIONS * SAMPLES * 4
            us = float(np.median(t_host[1:])) * 1e6
            host_inputs = {"us_per_report": round(us, 1), "host_bytes": nbytes, "gb_per_s": round(nbytes / us / 1e3, 2),
                           "note": "samples start in pageable host memory; per logical rank one H2D copy + one strided append of the [64, 10000] matrix, then the report; not the headline value"}
        except Exception as e:  # noqa: BLE001  (a side leg: see _side_leg)
            host_inputs = {"error": f"{type(e).__name__}: {str(e)[-300:]}"}

    cadence = None
    if args.full and world == 1 and not args.no_cadence:
        cadence = {"headline_workload": _side_leg(_cadence_leg, args.cadence_reports, job)}
        job.backend.synchronize()
        cadence.update(_side_leg(_cadence_leg, args.cadence_reports))

    per_kernel = None
    if args.full and world == 1 and not args.no_extra_legs:
        job.backend.synchronize()
        per_kernel = _side_leg(_per_kernel_leg)

    kernels_mode = None
    if args.full and world == 1 and not args.no_kernels_mode and not args.no_overhead:
        job.backend.synchronize()
        torch.cuda.synchronize()
        kernels_mode = _side_leg(_kernels_mode_leg)
        stamp_twin = _side_leg(_kernels_mode_leg, "stamp_mode")
        if isinstance(kernels_mode, dict) and isinstance(stamp_twin, dict):
            # the SAME workload on region stamps (single-process default): what of the figures above is the mode's doing
            kernels_mode["same_workload_on_region_stamps"] = {k: stamp_twin.get(k) for k in
                                                              ("per_step_overhead_kernels", "report_at_cadence_kernels", "error") if k in stamp_twin}

    overhead = overhead_async = None
    if args.full and not args.no_overhead:
        job.backend.synchronize()
        # (collective at N > 1: every rank runs it and a failure is a failure of the job; at N = 1 it is a side leg)
        if world == 1:
            overhead = _side_leg(_per_step_overhead, world, rank, args.overhead_steps, args.overhead_blocks)
            overhead_async = _side_leg(_per_step_overhead, world, rank, args.overhead_steps, args.overhead_blocks, asynchronous=True)
        else:
            overhead = _per_step_overhead(world, rank, args.overhead_steps, args.overhead_blocks)

    ex_us = exchange.get("us_median", 0.0) if exchange else 0.0
    if world > 1:
        elapsed, elapsed_instr, ex_us = times_max

    if rank == 0:
        us_per_report = elapsed / args.steps * 1e6
        out = {
            "metric": "generate_report_latency_us",
            "value": round(us_per_report, 2),
            "unit": "us",
            "n_gpus": distinct_devices,  # physical devices in use; == ranks on a node with one GPU per rank
            "ranks": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(us_per_report / 1e3, 5),
            "higher_is_better": False,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "config": {
                "workload": f"{TOTAL_RANKS} ranks x {SECTIONS} sections x {SAMPLES} samples per report, ring capacity {SAMPLES}, "
                            "relative+individual scores, gather_on_rank0",
                "logical_ranks_per_gpu": job.local_ranks,  # per process (== per GPU unless ranks share a device)
                "ranks_share_devices": distinct_devices < world,
                "rows_per_gpu": job.local_ranks * SECTIONS,
                "exchange": "none (single process)" if world == 1 else f"1 all-gather of {job.local_ranks}x{2 * SECTIONS + 1} f32 per rank ({getattr(job.reporter._direct, 'route', 'torch.distributed ' + args.backend)})",
                "target_us": 50,
            },
            "python": "%d.%d.%d" % sys.version_info[:3],  # (nvrx_pyread.c fills CPython 3.10's dict layout in place; any other version takes the public-API path)
            "gpu_timing_mode": _ktrace.timing_mode(),  # how profile_cuda sections would be timed in these processes (kernels = the default of multi-rank jobs)
            # why: this script selects its device BEFORE it imports the package (the headline path has no sections), so even
            # at N > 1 the per-step-overhead leg runs on region stamps; a job that imports nvrx_straggler first gets `kernels`
            "gpu_timing_mode_note": _ktrace.mode_note(),
            "reports_per_s": round(1e6 / us_per_report, 1),
            "us_per_report_median": round(float(np.median(per_step)) / 1e3, 2),
            "us_per_report_p95": round(float(np.percentile(per_step, 95)) / 1e3, 2),
            "us_per_call_median": round(call_us_median, 2),  # re-arm + generate_report() alone inside the same timed steps
            # what separates `value` (the whole bracketed region / K) from the median step: the first step after the opening
            # device synchronize, and the closing synchronize itself (a marker on every queue the reports used: ~12 us per
            # stream even when its work is long done), both divided by K
            "timed_region": {"first_step_us": round(per_step[0] / 1e3, 2), "closing_synchronize_us": round(closing_sync_us, 2),
                             "sum_of_steps_us": round(sum(per_step) / 1e3, 2), "region_us": round(elapsed * 1e6, 2)},
        }
        if args.full:
            kern_us = kern_total_us / max(kern_launches, 1)
            alg_bytes = job.local_ranks * SECTIONS * SAMPLES * 4
            achieved = alg_bytes / (kern_us * 1e-6) / 1e9 if kern_us > 0 else 0.0
            out["instrumented_ms_per_step"] = round(elapsed_instr / args.steps * 1e3, 5)
            out["roofline"] = {
                "bound": "hbm",
                "kernel": "k_row_stats",
                "achieved": round(achieved, 1),
                "peak": HBM_PEAK_GBS,
                "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBS, 4),
                "traffic": _pmc_traffic(job.local_ranks * SECTIONS),
                "traffic_of_an_older_source": _pmc_traffic_of_an_older_source(job.local_ranks * SECTIONS),
                "algorithmic_bytes_per_launch": alg_bytes,
                "kernel_us_avg": round(kern_us, 3),
                "launches_timed": kern_launches,
                "note": "hipExtLaunchKernel start/stop events on the launch stream. With the score kernel resident on its own "
                        "stream k_row_stats has no queued neighbour; under rocprofv3 the same launches read ~1 us longer, "
                        "because the profiler's own packets behind every dispatch are queued successors (DESIGN.md 3.5, "
                        "kbench between-launch modes)",
            }
        if score_tail:
            out["score_kernel"] = {
                "waited_for_rows_us": round(float(np.median(score_wait)) / 100.0, 2),
                "last_row_to_completion_word_us": round(float(np.median(score_tail)) / 100.0, 2),
                "last_row_to_scores_staged_us": round(float(np.median(score_staged)) / 100.0, 2),
                "note": "device clocks of the score kernel: resident on its own stream it waits for the statistics kernel's "
                        "granules; queued behind it (or behind an RCCL exchange) the first figure is ~0 and the second "
                        "is the kernel's whole body",
            }
        if report_read is not None:
            fully = us_per_report + report_read["all_six_mappings_us"]
            out["report_read"] = report_read
            out["us_per_report_fully_read"] = round(fully, 2)
        if args.dump_steps:
            out["per_step_us"] = [round(v / 1e3, 2) for v in per_step]
        if cadence is not None:
            out["report_at_cadence"] = cadence
        if per_kernel is not None:
            out["per_kernel_mode"] = per_kernel
        if cold is not None:
            out["roofline"]["cold"] = cold
        if n8 is not None:
            out["roofline_n8_shape"] = n8
        if detector_leg is not None:
            out["detector_report"] = detector_leg
        if section_entry is not None:
            out["section_entry_us"] = section_entry
        if overhead is not None:
            out["per_step_overhead"] = overhead
        if overhead_async is not None:
            out["per_step_overhead_async"] = overhead_async
        if kernels_mode is not None:
            # the mode every multi-rank job runs in: measured in a child interpreter that registered the tracer before HIP started
            for k in ("per_step_overhead_kernels", "report_at_cadence_kernels", "error"):
                if k in kernels_mode:
                    out[k if k != "error" else "kernels_mode_error"] = kernels_mode[k]
            twin = kernels_mode.get("same_workload_on_region_stamps") or {}
            if "per_step_overhead_kernels" in twin:
                out["per_step_overhead_transformer_on_region_stamps"] = twin["per_step_overhead_kernels"]
            if "report_at_cadence_kernels" in twin:
                out["report_at_cadence_transformer_on_region_stamps"] = twin["report_at_cadence_kernels"]
            out["kernels_mode_registered_through"] = kernels_mode.get("registered_through")
        if host_inputs is not None:
            out["host_inputs"] = host_inputs
        if exchange is not None:
            # latency-bound: 516 B x local ranks per rank over xGMI is far below a microsecond of wire time, so this
            # is RCCL's small-message launch + completion latency, not a bandwidth figure
            exchange["us_median"] = round(ex_us, 2) if "us_median" in exchange else None
            exchange["note"] = "enqueue + stream wait of one all-gather of the exchange rows, max over ranks; latency-bound"
            out["exchange"] = exchange
        if args.full and not args.no_cpu_baseline:
            # (at N > 1 the other ranks wait at the barrier below meanwhile: the baseline runs on rank 0's host cores)
            out["cpu_baseline"] = _side_leg(_cpu_baseline, args.cpu_reps)
    else:
        out = None

    # The line is printed exactly once: after the route legs (N > 1), by their watchdog if one of them does not come back, or --
    # if this process DIES in a leg (none of the in-stream routes has run across two real devices: a fault inside RCCL or an IPC
    # mapping is a signal, not an exception) -- by a sidecar that holds the headline line and prints it when our pipe closes.
    import threading

    printed = threading.Lock()
    sidecar = None
    if args.full and rank == 0 and world > 1 and not args.no_routes:
        sidecar = _headline_sidecar(out, job.reporter.exchange_info.get("mode", "c10d"))

    def emit(routes=None):
        if not printed.acquire(blocking=False):
            return
        if rank == 0:
            if sidecar is not None:
                try:
                    sidecar.stdin.write(b"DONE\n")
                    sidecar.stdin.close()
                    sidecar.wait(timeout=10)
                except Exception:  # noqa: BLE001
                    pass
            if routes is not None:
                mode = job.reporter.exchange_info.get("mode", "c10d")
                head = {"us_median": out["us_per_report_median"], "status": "ok (the headline of this line)",
                        "ran_on": getattr(job.reporter._direct, "route", None) or job.reporter.exchange_info.get("route", "torch.distributed")}
                if exchange and "floor_us" in exchange:
                    head["floor_us"] = exchange["floor_us"]
                out["routes"] = {mode: head, **routes}
            print(json.dumps(out), flush=True)

    clean = True
    if args.full and world > 1 and not args.no_routes:
        dist.barrier()  # (rank 0 comes from its CPU baseline: the legs' deadlines start together)
        headline_mode = job.reporter.exchange_info.get("mode", "c10d") if job.reporter._direct is None else job.reporter.exchange_info.get("mode", "rccl")
        routes, clean = _routes_table(world, rank, min(args.steps, 100), min(args.warmup, 10), headline_mode, args.route_timeout, emit)
        emit(routes)
    else:
        emit()
    if not clean:
        # a leg failed on this rank: its peers are still inside that leg's collectives (their watchdogs end them); nothing can be
        # torn down in order any more
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(0)
    if world > 1:
        # the line is out; a peer that left through its watchdog (or died) must not keep this rank in the closing barrier for the
        # process group's ten-minute timeout
        bye = threading.Timer(120.0, lambda: os._exit(0))
        bye.daemon = True
        bye.start()
    job.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
