#!/usr/bin/env python3
"""What the timeline scores cost (docs/MEASUREMENTS.md, "Timeline scores").  One GPU:

    python tools/timeline_cost.py kernels [--launches 200] [--warmup 10] [--repeats 5]
    python tools/timeline_cost.py report  [--reports 50] [--warmup 5]

``kernels``: ``k_row_timeline`` (B = 32) next to ``k_row_stats`` and ``k_row_onset`` on the SAME rows, alternating in one run --
    512 x 10 000 (8 ranks x 64 sections folded on one GPU) and 64 x 10 000 (one rank's); then ``k_timeline_rank`` and
    ``k_timeline_score`` at ranks x columns = 8 x 64, 8 x 4096 and 1024 x 128.  Prints hipEvent microseconds per launch
    (back-to-back launches: throughput, not latency; the median of ``--repeats`` windows of ``--launches``).
``report``: ``generate_report_from_rings`` + ``identify_stragglers()`` of the headline shape (8 folded ranks x 64 sections x
    10 000 samples) with ``timeline_scores`` off and on, alternating in one process, median and p95 of ``--reports`` each; with
    the option on also the time until ``timeline_scores()`` has returned.
Prints one JSON line per measurement.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "nvidia-resiliency-ext_amd"), REPO]

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROW_SHAPES = [(512, 10000), (64, 10000)]
RANK_SHAPES = [(8, 64), (8, 4096), (1024, 128)]  # ranks x columns (all of them kernel columns)
B = 32


def _timed(fn, launches, stream):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    for _ in range(launches):
        fn()
    t1.record(stream)
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / launches


def _alternating(launch, args, stream, sync):
    us = {name: [] for name in launch}
    for name in us:
        for _ in range(args.warmup):
            launch[name]()
    sync()
    for _ in range(args.repeats):
        for name in us:
            us[name].append(_timed(launch[name], args.launches, stream))
    out = {}
    for name in us:
        out[f"{name}_us"] = round(float(np.median(us[name])), 2)
        out[f"{name}_spread_us"] = [round(min(us[name]), 2), round(max(us[name]), 2)]
    return out


def kernels(args):
    from nvrx_straggler import _native
    from nvrx_straggler.backend import get_backend

    torch.cuda.set_device(0)
    be = get_backend()
    lib, st = be.lib, be.stream_handle
    rng = np.random.default_rng(0)
    for rows, n in ROW_SHAPES:
        with torch.cuda.stream(be.stream):
            samples = torch.from_numpy(rng.lognormal(np.log(1000.0), 0.02, (rows, n)).astype(np.float32)).to(be.device)
            counts = torch.full((rows,), n, dtype=torch.int32, device=be.device)
            stats = torch.empty((rows, _native.STATS_STRIDE), dtype=torch.float32, device=be.device)
            onsets = torch.empty((rows, 4), dtype=torch.int32, device=be.device)
            out = torch.empty((B, rows), dtype=torch.float32, device=be.device)
        be.synchronize()
        s, c = samples.data_ptr(), counts.data_ptr()
        launch = {
            "row_timeline": lambda: _native.check(lib.nvrx_row_timeline(s, c, None, rows, n, B, out.data_ptr(), st)),
            "row_stats": lambda: _native.check(lib.nvrx_row_stats(s, c, None, rows, n, stats.data_ptr(), st)),
            "row_onset": lambda: _native.check(lib.nvrx_row_onset(s, c, None, rows, n, 50000, onsets.data_ptr(), st)),
        }
        res = {"what": "row kernels", "rows": rows, "samples": n, "B": B, "launches": args.launches, "repeats": args.repeats}
        res.update(_alternating(launch, args, be.stream, be.synchronize))
        print(json.dumps(res), flush=True)
    for ranks, cols in RANK_SHAPES:
        with torch.cuda.stream(be.stream):
            planes = torch.from_numpy((1.0 + 0.01 * rng.standard_normal((ranks, B, cols))).astype(np.float32)).to(be.device)
            blocks = torch.empty((ranks, 2, 3, B), dtype=torch.float32, device=be.device)
            records = torch.empty((ranks, 2, 4 + B), dtype=torch.int32, device=be.device)
        be.synchronize()
        launch = {
            "timeline_rank": lambda: _native.check(lib.nvrx_timeline_rank(planes.data_ptr(), ranks, B, cols, 0, 30000,
                                                                          blocks.data_ptr(), st)),
            "timeline_score": lambda: _native.check(lib.nvrx_timeline_score(blocks.data_ptr(), ranks, B, 0, ranks, 8, 30000, 900000,
                                                                            records.data_ptr(), st)),
        }
        res = {"what": "rank and score kernels", "ranks": ranks, "columns": cols, "B": B, "launches": args.launches,
               "repeats": args.repeats}
        res.update(_alternating(launch, args, be.stream, be.synchronize))
        print(json.dumps(res), flush=True)


def report(args):
    torch.cuda.set_device(0)
    from nvrx_straggler import _native
    from nvrx_straggler.backend import get_backend
    from nvrx_straggler.reporting import ReportGenerator

    be = get_backend()
    local_ranks, sections, samples = 8, 64, 10_000
    rings = be.make_rings(local_ranks, sections, samples)
    srows = {f"section_{i:03d}": rings.row_for(_native.KIND_SECTION, f"section_{i:03d}") for i in range(sections)}
    rng = np.random.default_rng(0)
    for lr in range(local_ranks):
        data = rng.lognormal(np.log(1000.0), 0.02, (sections, samples)).astype(np.float32)
        rings.push_device_rows(0, torch.from_numpy(data).to(be.device), lr=lr)
    be.synchronize()
    torch.cuda.synchronize()
    gens = {0: ReportGenerator(["relative_perf_scores"], node_name="n"),
            1: ReportGenerator(["relative_perf_scores"], node_name="n", timeline_scores=True)}
    lat, readable = {0: [], 1: []}, []
    try:
        for i in range(2 * (args.reports + args.warmup)):
            on = i & 1
            rings.set_count_all(samples)
            t0 = time.perf_counter_ns()
            rep = gens[on].generate_report_from_rings(rings, srows, {}, local_ranks=local_ranks)
            rep.identify_stragglers()
            t1 = time.perf_counter_ns()
            if on:
                assert len(rep.timeline_scores()["ranks"]) == local_ranks
            t2 = time.perf_counter_ns()
            if i >= 2 * args.warmup:
                lat[on].append((t1 - t0) * 1e-3)
                if on:
                    readable.append((t2 - t0) * 1e-3)
            be.synchronize()
        out = {"what": "ring report, call -> flagged set", "reports_each": args.reports, "shape": "8 x 64 x 10000"}
        for on, key in ((0, "off"), (1, "on")):
            out[f"{key}_median_us"] = round(float(np.median(lat[on])), 1)
            out[f"{key}_p95_us"] = round(float(np.percentile(lat[on], 95)), 1)
        out["delta_median_us"] = round(out["on_median_us"] - out["off_median_us"], 1)
        out["timeline_readable_median_us"] = round(float(np.median(readable)), 1)
        print(json.dumps(out), flush=True)
    finally:
        for g in gens.values():
            g.close()
        rings.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "report"])
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--reports", type=int, default=50)
    args = ap.parse_args()
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    {"kernels": kernels, "report": report}[args.what](args)


if __name__ == "__main__":
    main()
