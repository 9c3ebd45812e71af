#!/usr/bin/env python3
"""What episode scores cost (docs/MEASUREMENTS.md, "Episode scores").  One GPU:

    python tools/episode_cost.py kernels [--launches 20] [--warmup 3]
    python tools/episode_cost.py report  [--reports 50] [--warmup 5] [--ranks 1|2] [--asynchronous]

``kernels``: ``k_row_episode`` (``min_len_ppm`` 5000, the default, and 333 333, where the lagged stream starts a third of the
    row behind) and ``k_row_onset`` beside it for scale, on the SAME rows in the same run -- 512 x 10 000 (8 ranks x 64
    sections folded on one GPU) and 64 x 10 000 (one rank's) -- ``--launches`` each after ``--warmup``.  Prints hipEvent
    microseconds per launch (back-to-back launches: throughput, not latency) and the ratio to ``k_row_onset``.  The episode
    kernel reads a row about four times where the onset kernel reads it twice, the fourth time with 4-byte loads, and runs
    three scans per 256 samples where the onset kernel runs one.
``report``: ``generate_report_from_rings`` + ``identify_stragglers()`` of the headline shape (8 folded ranks x 64 sections x
    10 000 samples) with ``episode_detection`` off and on, alternating in one process, median and p95 of ``--reports`` each;
    with the option on also the time until ``episode_scores()`` has returned.  ``--asynchronous``: both generators enqueue
    only.  ``--ranks 2``: two gloo processes sharing the GPU, four folded ranks each; rank 0 prints.
Prints one JSON line per measurement.
"""
import argparse
import json
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "nvidia-resiliency-ext_amd"), REPO]

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = [(512, 10000), (64, 10000)]


def _timed(fn, launches, warmup, stream):
    for _ in range(warmup):
        fn()
    stream.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    for _ in range(launches):
        fn()
    t1.record(stream)
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / launches


def kernels(args):
    from nvrx_straggler import _native
    from nvrx_straggler.backend import get_backend

    torch.cuda.set_device(0)
    be = get_backend()
    lib, st = be.lib, be.stream_handle
    rng = np.random.default_rng(0)
    for rows, n in SHAPES:
        with torch.cuda.stream(be.stream):
            samples = torch.from_numpy(rng.lognormal(np.log(1000.0), 0.02, (rows, n)).astype(np.float32)).to(be.device)
            counts = torch.full((rows,), n, dtype=torch.int32, device=be.device)
            onsets = torch.empty((rows, 4), dtype=torch.int32, device=be.device)
            episodes = torch.empty((rows, 4), dtype=torch.int32, device=be.device)
        be.synchronize()

        def row_onset():
            _native.check(lib.nvrx_row_onset(samples.data_ptr(), counts.data_ptr(), None, rows, n, 50000, onsets.data_ptr(), st))

        def row_episode(len_ppm):
            def launch():
                _native.check(lib.nvrx_row_episode(samples.data_ptr(), counts.data_ptr(), None, rows, n, len_ppm,
                                                   episodes.data_ptr(), st))
            return launch

        out = {"what": "kernels", "rows": rows, "samples": n, "launches": args.launches}
        out["row_onset_us"] = round(_timed(row_onset, args.launches, args.warmup, be.stream), 2)
        for len_ppm in (5000, 333333):
            out[f"row_episode_{len_ppm}_us"] = round(_timed(row_episode(len_ppm), args.launches, args.warmup, be.stream), 2)
            out[f"ratio_{len_ppm}"] = round(out[f"row_episode_{len_ppm}_us"] / out["row_onset_us"], 2)
        print(json.dumps(out), flush=True)


def _report_worker(rank, world, store, args):
    if world > 1:
        os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1")
        torch.distributed.init_process_group("gloo", init_method=f"file://{store}", world_size=world, rank=rank)
    torch.cuda.set_device(0)
    from nvrx_straggler import _native
    from nvrx_straggler.backend import get_backend
    from nvrx_straggler.reporting import ReportGenerator

    be = get_backend()
    local_ranks, sections, samples = 8 // world, 64, 10_000
    rings = be.make_rings(local_ranks, sections, samples)
    srows = {f"section_{i:03d}": rings.row_for(_native.KIND_SECTION, f"section_{i:03d}") for i in range(sections)}
    krows = {}
    rng = np.random.default_rng(rank)
    for lr in range(local_ranks):
        data = rng.lognormal(np.log(1000.0), 0.02, (sections, samples)).astype(np.float32)
        rings.push_device_rows(0, torch.from_numpy(data).to(be.device), lr=lr)
    be.synchronize()
    torch.cuda.synchronize()
    gens = {0: ReportGenerator(["relative_perf_scores"], node_name="n", asynchronous=args.asynchronous),
            1: ReportGenerator(["relative_perf_scores"], node_name="n", asynchronous=args.asynchronous, episode_detection=True)}
    lat, readable = {0: [], 1: []}, []
    try:
        for i in range(2 * (args.reports + args.warmup)):
            on = i & 1
            rings.set_count_all(samples)
            t0 = time.perf_counter_ns()
            rep = gens[on].generate_report_from_rings(rings, srows, krows, local_ranks=local_ranks)
            if rep is not None:
                rep.identify_stragglers()
            t1 = time.perf_counter_ns()
            if on and rep is not None:
                assert len(rep.episode_scores()["section_relative"]) == sections
            t2 = time.perf_counter_ns()
            if i >= 2 * args.warmup:
                lat[on].append((t1 - t0) * 1e-3)
                if on:
                    readable.append((t2 - t0) * 1e-3)
            be.synchronize()
        if rank == 0:
            out = {"what": "ring report, call -> flagged set", "processes": world, "reports_each": args.reports,
                   "shape": "8 x 64 x 10000", "asynchronous": bool(args.asynchronous)}
            for on, key in ((0, "off"), (1, "on")):
                out[f"{key}_median_us"] = round(float(np.median(lat[on])), 1)
                out[f"{key}_p95_us"] = round(float(np.percentile(lat[on], 95)), 1)
            out["delta_median_us"] = round(out["on_median_us"] - out["off_median_us"], 1)
            out["episodes_readable_median_us"] = round(float(np.median(readable)), 1)
            print(json.dumps(out), flush=True)
    finally:
        for g in gens.values():
            g.close()
        rings.close()
        if world > 1:
            torch.distributed.barrier()
            torch.distributed.destroy_process_group()


def report(args):
    if args.ranks == 1:
        _report_worker(0, 1, None, args)
        return
    import torch.multiprocessing as mp

    with tempfile.NamedTemporaryFile(delete=True) as f:
        store = f.name
    mp.spawn(_report_worker, args=(args.ranks, store, args), nprocs=args.ranks, join=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "report"])
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reports", type=int, default=50)
    ap.add_argument("--asynchronous", action="store_true")
    ap.add_argument("--ranks", type=int, default=1, choices=[1, 2, 4, 8])
    args = ap.parse_args()
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    {"kernels": kernels, "report": report}[args.what](args)


if __name__ == "__main__":
    main()
