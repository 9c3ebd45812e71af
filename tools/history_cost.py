#!/usr/bin/env python3
"""What the score history costs (docs/MEASUREMENTS.md, "Score history").  One GPU:

    python tools/history_cost.py kernels [--launches 200] [--warmup 20]
    python tools/history_cost.py report  [--reports 200] [--warmup 20]

``kernels``: ``nvrx_score_history`` (``k_score_history``, every rank reported) on random score rows of (ranks, section ids,
    depth) = (8, 64, 8), (64, 64, 64) and (1024, 64, 8), ``--launches`` each after ``--warmup``, the ring wrapping as it goes;
    next to it, in the same run and on the same ranks x section ids, ``nvrx_robust_score`` (``k_robust_cols`` +
    ``k_robust_rank``), the sibling of comparable size.  Prints hipEvent microseconds per call (back-to-back: throughput, not
    latency); for per-dispatch durations run it under the profiler, alone:
    ``rocprofv3 --kernel-trace --stats -d <dir> -- python tools/history_cost.py kernels``.
``report``: ``generate_report_from_rings`` + ``identify_stragglers()`` of the headline shape (8 folded ranks x 64 sections x
    10 000 samples), synchronous, with ``score_history`` off and on (8 reports deep), alternating in one process (off on on
    off ...), median and p95 of ``--reports`` each; with the option on also the time until
    ``identify_persistent_stragglers()`` has returned.
Prints one JSON line per measurement.
"""
import argparse
import ctypes
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "nvidia-resiliency-ext_amd"), REPO]

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = [(8, 64, 8), (64, 64, 64), (1024, 64, 8)]  # (ranks, section ids, depth)


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
    thr = (ctypes.c_double * 4)(0.75, 0.75, 0.75, 0.75)
    for R, S, H in SHAPES:
        with torch.cuda.stream(be.stream):
            scores = torch.from_numpy(rng.uniform(0.5, 1.0, (R, _native.score_len(S))).astype(np.float32)).to(be.device)
            ring = torch.full((_native.history_floats(R, S, H) * 4,), 0xFF, dtype=torch.uint8, device=be.device)
            out = torch.empty(_native.history_words(R, S), dtype=torch.int32, device=be.device)
            # the sibling's input: an exchange table of the same ranks x section ids (no kernel ids)
            table = np.zeros((R, _native.table_len(0, S)), dtype=np.float32)
            table[:, :S] = rng.lognormal(np.log(1000.0), 0.05, (R, S))
            table[:, S : 2 * S] = table[:, :S] * 0.9
            table[:, -1] = 1.0
            d_table = torch.from_numpy(table).to(be.device)
            robust_out = torch.empty(_native.robust_words(R, 0, S), dtype=torch.int32, device=be.device)
        be.synchronize()
        n = [0]

        def history():
            _native.check(lib.nvrx_score_history(scores.data_ptr(), R, S, 0, R, ring.data_ptr(), S, H, n[0], thr,
                                                 out.data_ptr(), st))
            n[0] += 1

        def robust():
            _native.check(lib.nvrx_robust_score(d_table.data_ptr(), R, 0, S, 0, R, 4, 0.02, robust_out.data_ptr(), st))

        res = {"what": "kernels", "ranks": R, "section_ids": S, "depth": H, "launches": args.launches}
        # alternating rounds in one process: the spread between rounds says what a difference is worth
        rounds = {"history_us": [], "robust_pair_us": []}
        for _ in range(3):
            rounds["history_us"].append(_timed(history, args.launches, args.warmup, be.stream))
            rounds["robust_pair_us"].append(_timed(robust, args.launches, args.warmup, be.stream))
        for key, vals in rounds.items():
            res[key] = round(float(np.median(vals)), 2)
            res[key + "_rounds"] = [round(v, 2) for v in vals]
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
    krows = {}
    rng = np.random.default_rng(0)
    for lr in range(local_ranks):
        data = rng.lognormal(np.log(1000.0), 0.02, (sections, samples)).astype(np.float32)
        rings.push_device_rows(0, torch.from_numpy(data).to(be.device), lr=lr)
    be.synchronize()
    torch.cuda.synchronize()
    gens = {0: ReportGenerator(["relative_perf_scores"], node_name="n"),
            1: ReportGenerator(["relative_perf_scores"], node_name="n", score_history=8, persistence_min_reports=3)}
    lat, readable = {0: [], 1: []}, []
    try:
        for i in range(2 * (args.reports + args.warmup)):
            on = (i ^ (i >> 1)) & 1  # off on on off ...: either setting follows itself as often as it follows the other
            rings.set_count_all(samples)
            t0 = time.perf_counter_ns()
            rep = gens[on].generate_report_from_rings(rings, srows, krows, local_ranks=local_ranks)
            rep.identify_stragglers()
            t1 = time.perf_counter_ns()
            if on:
                rep.identify_persistent_stragglers()
            t2 = time.perf_counter_ns()
            if i >= 2 * args.warmup:
                lat[on].append((t1 - t0) * 1e-3)
                if on:
                    readable.append((t2 - t0) * 1e-3)
            be.synchronize()
        out = {"what": "ring report, call -> flagged set", "processes": 1, "reports_each": args.reports, "shape": "8 x 64 x 10000",
               "depth": 8}
        for on, key in ((0, "off"), (1, "on")):
            out[f"{key}_median_us"] = round(float(np.median(lat[on])), 1)
            out[f"{key}_p95_us"] = round(float(np.percentile(lat[on], 95)), 1)
        out["delta_median_us"] = round(out["on_median_us"] - out["off_median_us"], 1)
        out["persistent_readable_median_us"] = round(float(np.median(readable)), 1)
        print(json.dumps(out), flush=True)
    finally:
        for g in gens.values():
            g.close()
        rings.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "report"])
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reports", type=int, default=200)
    args = ap.parse_args()
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    {"kernels": kernels, "report": report}[args.what](args)


if __name__ == "__main__":
    main()
