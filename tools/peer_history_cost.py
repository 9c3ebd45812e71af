#!/usr/bin/env python3
"""What the peer-score history and trends cost (docs/MEASUREMENTS.md, "Peer history").  One GPU:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/peer_history_cost.py kernels [--launches 200]
    python tools/peer_history_cost.py report [--reports 200] [--warmup 20]

``kernels``: meant to run under ``rocprofv3 --kernel-trace --stats`` (a run of its own: no counters, no other tracing), whose
    statistics give the time per dispatch.  Per shape -- (ranks, section ids, depth) = (8, 64, 8) and (1024, 64, 16) -- a ring
    of each kind is filled by 2 x depth steps on random scores, then ``--launches`` rounds of the four steps follow each
    other: ``nvrx_peer_history``, ``nvrx_score_history``, ``nvrx_peer_trend``, ``nvrx_score_trend`` (``--score-first``: each
    pair the other way round -- at the small shape a dispatch's time depends on what ran before it).  The shapes run one after
    the other, so the statistics mix them per kernel name; the kernel trace itself (``*_kernel_trace.csv``) keeps every
    dispatch with its grid size, by which ``--summarise <csv>`` tells the shapes apart and prints the median per kernel and
    shape.  Without the profiler it prints hipEvent microseconds per call (back-to-back: throughput, not latency).
``report``: ``generate_report_from_rings`` + ``identify_peer_stragglers()`` of the headline shape (8 folded ranks x 64
    sections x 10 000 samples, ``peer_groups="block:4"``), synchronous, ``peer_history`` off and on (depth 8) in one process
    in the order off on on off ..., median and p95 of ``--reports`` each; with the option on also the time until
    ``identify_persistent_peer_stragglers()`` has returned.
Prints one JSON line per measurement.
"""
import argparse
import csv
import ctypes
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "nvidia-resiliency-ext_amd"), REPO]

import numpy as np  # noqa: E402

SHAPES = [(8, 64, 8), (1024, 64, 16)]  # (ranks, section ids, depth)


def _waves(R, S, H, fams):
    per_wave = 64 // (16 if H <= 16 else 32 if H <= 32 else 64)
    return R * fams * -(-(1 + S) // per_wave)


def kernels(args):
    import torch

    from nvrx_straggler import _native
    from nvrx_straggler.backend import get_backend

    torch.cuda.set_device(0)
    be = get_backend()
    lib, st = be.lib, be.stream_handle
    rng = np.random.default_rng(0)
    thr2, thr4 = (ctypes.c_double * 2)(0.75, 0.75), (ctypes.c_double * 4)(0.75, 0.75, 0.75, 0.75)
    for R, S, H in SHAPES:
        with torch.cuda.stream(be.stream):
            rows = [torch.from_numpy(rng.uniform(0.5, 1.0, (R, _native.score_len(S))).astype(np.float32)).to(be.device)
                    for _ in range(7)]
            planes = [torch.from_numpy(rng.uniform(0.5, 1.0, (R, 1 + S)).astype(np.float32)).to(be.device) for _ in range(7)]
            ring = torch.full((_native.history_floats(R, S, H) * 4,), 0xFF, dtype=torch.uint8, device=be.device)
            peer_ring = torch.full((_native.peer_history_floats(R, S, H) * 4,), 0xFF, dtype=torch.uint8, device=be.device)
            out = torch.empty(_native.history_words(R, S), dtype=torch.int32, device=be.device)
        be.synchronize()
        n = [0]

        def steps():
            k = n[0]
            calls = [lambda: lib.nvrx_peer_history(planes[k % 7].data_ptr(), R, S, peer_ring.data_ptr(), S, H, k, thr2, out.data_ptr(), st),
                     lambda: lib.nvrx_score_history(rows[k % 7].data_ptr(), R, S, 0, R, ring.data_ptr(), S, H, k, thr4, out.data_ptr(), st),
                     lambda: lib.nvrx_peer_trend(peer_ring.data_ptr(), R, S, S, H, k + 1, out.data_ptr(), st),
                     lambda: lib.nvrx_score_trend(ring.data_ptr(), R, S, S, H, k + 1, out.data_ptr(), st)]
            for i in ((1, 0, 3, 2) if args.score_first else (0, 1, 2, 3)):
                _native.check(calls[i]())
            n[0] += 1

        for _ in range(2 * H):
            steps()
        be.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(be.stream)
        for _ in range(args.launches):
            steps()
        t1.record(be.stream)
        t1.synchronize()
        print(json.dumps({"what": "kernels", "ranks": R, "section_ids": S, "depth": H, "rounds": args.launches,
                          "four_steps_us": round(t0.elapsed_time(t1) * 1e3 / args.launches, 2),
                          "workgroups": {"peer": -(-_waves(R, S, H, 1) // 4), "score": -(-_waves(R, S, H, 2) // 4)}}), flush=True)


def summarise(path):
    """Median duration per kernel and grid size of a rocprofv3 kernel trace (the grid tells the two shapes apart)."""
    groups = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"]
            short = next((k for k in ("k_peer_history", "k_score_history", "k_peer_trend", "k_score_trend") if k in name), None)
            if short is None:
                continue
            grid = int(row.get("Grid_Size", row.get("Grid_Size_X", 0)) or 0)
            groups.setdefault((short, grid), []).append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
    for (short, grid), ns in sorted(groups.items()):
        a = np.array(ns, dtype=np.float64) / 1e3
        print(json.dumps({"what": "kernel trace", "kernel": short, "grid_threads": grid, "dispatches": int(a.size),
                          "median_us": round(float(np.median(a)), 2), "p5_us": round(float(np.percentile(a, 5)), 2),
                          "p95_us": round(float(np.percentile(a, 95)), 2)}), flush=True)


def report(args):
    import torch

    torch.cuda.set_device(0)
    from nvrx_straggler import _native
    from nvrx_straggler.backend import get_backend
    from nvrx_straggler.reporting import ReportGenerator

    be = get_backend()
    local_ranks, sections, samples = 8, 64, 10_000
    rings = be.make_rings(local_ranks, sections, samples)
    srows = {f"section_{i:03d}": rings.row_for(_native.KIND_SECTION, f"section_{i:03d}") for i in range(sections)}
    krows = {}  # (the same objects every report: the generators keep their plans)
    rng = np.random.default_rng(0)
    for lr in range(local_ranks):
        data = rng.lognormal(np.log(1000.0), 0.02, (sections, samples)).astype(np.float32)
        rings.push_device_rows(0, torch.from_numpy(data).to(be.device), lr=lr)
    be.synchronize()
    torch.cuda.synchronize()
    names = ("off", "on")
    gens = {"off": ReportGenerator(["relative_perf_scores"], node_name="n", peer_groups="block:4"),
            "on": ReportGenerator(["relative_perf_scores"], node_name="n", peer_groups="block:4", peer_history=8,
                                  peer_persistence_min_reports=3)}
    lat, readable = {k: [] for k in names}, []
    order = (0, 1, 1, 0)  # either setting follows itself as often as the other
    try:
        for i in range(2 * (args.reports + args.warmup)):
            key = names[order[i % 4]]
            rings.set_count_all(samples)
            t0 = time.perf_counter_ns()
            rep = gens[key].generate_report_from_rings(rings, srows, krows, local_ranks=local_ranks)
            rep.identify_peer_stragglers()
            t1 = time.perf_counter_ns()
            if key == "on":
                rep.identify_persistent_peer_stragglers()
            t2 = time.perf_counter_ns()
            if i >= 2 * args.warmup:
                lat[key].append((t1 - t0) * 1e-3)
                if key == "on":
                    readable.append((t2 - t0) * 1e-3)
            be.synchronize()
        out = {"what": "ring report with peer groups, call -> peer verdict", "processes": 1, "reports_each": args.reports,
               "shape": "8 x 64 x 10000", "depth": 8}
        for key in names:
            out[f"{key}_median_us"] = round(float(np.median(lat[key])), 1)
            out[f"{key}_p95_us"] = round(float(np.percentile(lat[key], 95)), 1)
        out["delta_median_us"] = round(out["on_median_us"] - out["off_median_us"], 1)
        out["persistent_readable_median_us"] = round(float(np.median(readable)), 1)
        print(json.dumps(out), flush=True)
    finally:
        for g in gens.values():
            g.close()
        rings.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "report", "summarise"])
    ap.add_argument("trace", nargs="?", help="summarise: the *_kernel_trace.csv rocprofv3 wrote")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--score-first", action="store_true", help="kernels: the score ring's step ahead of the peer ring's in each pair")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reports", type=int, default=200)
    args = ap.parse_args()
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if args.what == "summarise":
        summarise(args.trace)
        return
    {"kernels": kernels, "report": report}[args.what](args)


if __name__ == "__main__":
    main()
