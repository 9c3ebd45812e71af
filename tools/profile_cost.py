#!/usr/bin/env python3
"""What the tail profile costs (docs/MEASUREMENTS.md, "Tail profile").  One GPU:

    python tools/profile_cost.py kernels [--launches 200] [--warmup 10] [--repeats 5]
    python tools/profile_cost.py report  [--reports 50] [--warmup 5]

``kernels``: one ``k_row_profile`` launch of Q quantiles next to the only other way to get them, Q ``k_row_quantile`` launches
    on the SAME rows, alternating in one run, at Q = 3 and Q = 7 -- 512 x 10 000 (8 ranks x 64 sections folded on one GPU) and
    64 x 10 000 (one rank's), where the profile kernel keeps the first 8960 keys of a row in LDS, and 512 / 64 x 8192, where
    it keeps them all.  Prints hipEvent microseconds per launch (back-to-back launches: throughput, not latency; the median of
    ``--repeats`` windows of ``--launches``) and the ratio profile / (Q x quantile).
``report``: ``generate_report_from_rings`` + ``identify_stragglers()`` of the headline shape (8 folded ranks x 64 sections x
    10 000 samples) with ``tail_profile`` off and on at (0.9, 0.99, 0.999), alternating in one process, median and p95 of
    ``--reports`` each; with the option on also the time until ``tail_profile()`` has returned.
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

SHAPES = [(512, 10000), (64, 10000), (512, 8192), (64, 8192)]
Q_SETS = [(900000, 990000, 999000), (500000, 750000, 900000, 950000, 990000, 999000, 999900)]


def _timed(fn, launches, stream):
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
            out = torch.empty((_native.PROFILE_MAX_Q, rows), dtype=torch.float32, device=be.device)
        be.synchronize()
        s, c, o = samples.data_ptr(), counts.data_ptr(), out.data_ptr()
        for q_ppm in Q_SETS:
            q, Q = _native.q_array(q_ppm)
            launch = {
                "profile": lambda: _native.check(lib.nvrx_row_profile(s, c, rows, n, q, Q, o, st)),
                "quantile_xQ": lambda: [_native.check(lib.nvrx_row_quantile(s, c, rows, n, x, o, st)) for x in q_ppm],
            }
            us = {name: [] for name in launch}
            for name in us:
                for _ in range(args.warmup):
                    launch[name]()
            be.synchronize()
            for _ in range(args.repeats):
                for name in us:  # (alternating)
                    us[name].append(_timed(launch[name], args.launches, be.stream))
            res = {"what": "kernels", "rows": rows, "samples": n, "Q": Q, "launches": args.launches, "repeats": args.repeats,
                   "in_lds": n <= _native.PROFILE_LDS_SAMPLES}
            for name in us:
                res[f"{name}_us"] = round(float(np.median(us[name])), 2)
                res[f"{name}_spread_us"] = [round(min(us[name]), 2), round(max(us[name]), 2)]
            res["ratio"] = round(res["profile_us"] / res["quantile_xQ_us"], 3)
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
            1: ReportGenerator(["relative_perf_scores"], node_name="n", tail_profile=(0.9, 0.99, 0.999))}
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
                assert len(rep.tail_profile()["section_relative"]) == sections
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
        out["profile_readable_median_us"] = round(float(np.median(readable)), 1)
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
