#!/usr/bin/env python3
"""What score trends cost (docs/MEASUREMENTS.md, "Score trends").  One GPU:

    python tools/trend_cost.py kernels [--launches 200] [--warmup 20]
    python tools/trend_cost.py report  [--reports 200] [--warmup 20]
    python tools/trend_cost.py sketch  (NumPy only, no GPU: the table of DESIGN.md, "Score trends")

``kernels``: ``nvrx_score_trend`` (``k_score_trend``, every rank reported) next to ``nvrx_score_history``
    (``k_score_history``) on the SAME ring, (ranks, section ids, depth) = (8, 64, 8), (64, 64, 64) and (1024, 64, 8) -- the
    shapes of tools/history_cost.py.  The ring is first filled by 2 x depth history steps on random scores; then rounds of
    ``--launches`` history steps and ``--launches`` trend steps alternate in one process, three rounds each.  Prints hipEvent
    microseconds per call (back-to-back: throughput, not latency) and the ratio.
``report``: ``generate_report_from_rings`` + ``identify_stragglers()`` of the headline shape (8 folded ranks x 64 sections x
    10 000 samples), synchronous, in three configurations that alternate in one process -- both options off, the score history
    on (8 reports deep), history and trends on --, median and p95 of ``--reports`` each; with the trends on also the time
    until ``identify_declining_stragglers()`` has returned.
``sketch``: the shape of the effect on four illustrative series of 16 reports (seed 2026, 1 % noise), with the contract's
    arithmetic restated in NumPy: a score falling 0.012 per report, the same with one report at 0.60, a flat series with one
    window at 0.70 (next to its least-squares slope), and steady noise.
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
            # several score rows to cycle through, so that the ring holds a series and not one value
            rows = [torch.from_numpy(rng.uniform(0.5, 1.0, (R, _native.score_len(S))).astype(np.float32)).to(be.device)
                    for _ in range(7)]
            ring = torch.full((_native.history_floats(R, S, H) * 4,), 0xFF, dtype=torch.uint8, device=be.device)
            rec = torch.empty(_native.history_words(R, S), dtype=torch.int32, device=be.device)
            out = torch.empty(_native.trend_words(R, S), dtype=torch.int32, device=be.device)
        be.synchronize()
        n = [0]

        def history():
            _native.check(lib.nvrx_score_history(rows[n[0] % 7].data_ptr(), R, S, 0, R, ring.data_ptr(), S, H, n[0], thr,
                                                 rec.data_ptr(), st))
            n[0] += 1

        def trend():
            _native.check(lib.nvrx_score_trend(ring.data_ptr(), R, S, S, H, n[0], out.data_ptr(), st))

        for _ in range(2 * H):
            history()
        res = {"what": "kernels", "ranks": R, "section_ids": S, "depth": H, "launches": args.launches}
        rounds = {"history_us": [], "trend_us": []}
        for _ in range(3):  # alternating rounds in one process: the spread between rounds says what a difference is worth
            rounds["history_us"].append(_timed(history, args.launches, args.warmup, be.stream))
            rounds["trend_us"].append(_timed(trend, args.launches, args.warmup, be.stream))
        for key, vals in rounds.items():
            res[key] = round(float(np.median(vals)), 2)
            res[key + "_rounds"] = [round(v, 2) for v in vals]
        res["trend_over_history"] = round(res["trend_us"] / res["history_us"], 2)
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
    names = ("off", "history", "history_trends")
    gens = {"off": ReportGenerator(["relative_perf_scores"], node_name="n"),
            "history": ReportGenerator(["relative_perf_scores"], node_name="n", score_history=8, persistence_min_reports=3),
            "history_trends": ReportGenerator(["relative_perf_scores"], node_name="n", score_history=8, persistence_min_reports=3,
                                              score_trends=True)}
    lat, readable = {k: [] for k in names}, []
    order = (0, 1, 2, 2, 1, 0)  # every configuration follows itself and each of the others
    try:
        for i in range(3 * (args.reports + args.warmup)):
            key = names[order[i % 6]]
            rings.set_count_all(samples)
            t0 = time.perf_counter_ns()
            rep = gens[key].generate_report_from_rings(rings, srows, krows, local_ranks=local_ranks)
            rep.identify_stragglers()
            t1 = time.perf_counter_ns()
            if key == "history_trends":
                rep.identify_declining_stragglers()
            t2 = time.perf_counter_ns()
            if i >= 3 * args.warmup:
                lat[key].append((t1 - t0) * 1e-3)
                if key == "history_trends":
                    readable.append((t2 - t0) * 1e-3)
            be.synchronize()
        out = {"what": "ring report, call -> flagged set", "processes": 1, "reports_each": args.reports, "shape": "8 x 64 x 10000",
               "depth": 8}
        for key in names:
            out[f"{key}_median_us"] = round(float(np.median(lat[key])), 1)
            out[f"{key}_p95_us"] = round(float(np.percentile(lat[key], 95)), 1)
        out["trends_delta_median_us"] = round(out["history_trends_median_us"] - out["history_median_us"], 1)
        out["declining_readable_median_us"] = round(float(np.median(readable)), 1)
        print(json.dumps(out), flush=True)
    finally:
        for g in gens.values():
            g.close()
        rings.close()


def _theil_sen(x_oldest_first):
    """(slope, level, tau) of one series as include/nvrx_straggler.h defines them (nvrx_score_trend), newest entry at age 0."""
    x = np.asarray(x_oldest_first, dtype=np.float32)[::-1]
    a, b = np.triu_indices(x.size, 1)
    slopes = np.sort(((x[a].astype(np.float64) - x[b].astype(np.float64)) / (b - a)).astype(np.float32))
    slope = slopes[(slopes.size - 1) >> 1]
    v = np.sort((x.astype(np.float64) + np.float64(slope) * np.arange(x.size)).astype(np.float32))
    s = int(np.sign(x[a].astype(np.float64) - x[b].astype(np.float64)).sum())
    return float(slope), float(v[(x.size - 1) >> 1]), s / slopes.size


def sketch(args):
    rng = np.random.default_rng(2026)
    n = np.arange(16)
    noise = 0.01 * rng.standard_normal(16)
    falling = 0.97 - 0.012 * n + noise
    with_outlier = falling.copy()
    with_outlier[9] = 0.60
    flat = 0.95 + noise
    flat_outlier = flat.copy()
    flat_outlier[9] = 0.70
    for name, x in (("falling 0.012 per report", falling), ("the same, one report at 0.60", with_outlier),
                    ("flat, one window at 0.70", flat_outlier), ("steady noise", flat)):
        slope, level, tau = _theil_sen(x)
        left = None if not (slope < 0 and tau <= -0.6) else 0 if level < 0.75 else int(np.ceil((level - 0.75) / -slope))
        print(json.dumps({"what": "sketch", "series": name, "theil_sen_slope": round(slope, 4), "kendall_tau": round(tau, 2),
                          "least_squares_slope": round(float(np.polyfit(n, x, 1)[0]), 4), "latest": round(float(x[-1]), 3),
                          "lowest": round(float(x.min()), 3), "level": round(level, 3), "reports_left": left}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "report", "sketch"])
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reports", type=int, default=200)
    args = ap.parse_args()
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    {"kernels": kernels, "report": report, "sketch": sketch}[args.what](args)


if __name__ == "__main__":
    main()
