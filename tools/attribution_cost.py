#!/usr/bin/env python3
"""What kernel attribution costs (docs/MEASUREMENTS.md, "Kernel attribution").  One process, one GPU, one command:

    python tools/attribution_cost.py [--launches 200] [--warmup 20] [--reports 200]

(a) ``k_attribute`` (+ its column-minimum pass) next to ``nvrx_score`` ON THE SAME TABLE, hipEvents around ``--launches``
    back-to-back launches after ``--warmup`` warm-ups, microseconds per launch, for N = 5 and N = 16.  The score kernel is
    the yardstick: it reads the same table once.
(b) call -> flagged-set latency of a ring report whose table has kernels -- 8 folded ranks x (32 kernel + 32 section rows) x
    10 000 samples -- with the option off and on (N = 5), alternating in the same process: median and p95 of ``--reports``
    each; with the option on also the time from the call until ``explain_gpu_scores()`` has returned, and the latency of
    back-to-back reports whose attribution is never read (the next report then settles it first).
Prints one JSON line per measurement.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "nvidia-resiliency-ext_amd"), os.path.join(REPO, "tests"), REPO]

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = [(1, 3, 0), (8, 5, 6), (8, 4096, 8), (64, 17, 33), (100, 7, 9), (16, 13000, 40), (4096, 32, 16)]


def _random_table(rng, R, K, S, p_missing=0.15):
    KS, L = K + S, 2 * (K + S) + K + 1
    T = np.zeros((R, L), dtype=np.float32)
    med = rng.lognormal(1.0, 0.5, (R, KS)).astype(np.float32)
    hmin = (med * rng.uniform(0.5, 1.0, (R, KS))).astype(np.float32)
    missing = rng.random((R, KS)) < p_missing
    med[missing], hmin[missing] = -1.0, np.nan
    T[:, :KS], T[:, KS : 2 * KS] = med, hmin
    w = rng.uniform(1, 1000, (R, K)).astype(np.float32)
    w[missing[:, :K]] = 0.0
    T[:, 2 * KS : 2 * KS + K] = w
    T[:, L - 1] = 1.0
    return T


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


def operator_cost(be, launches, warmup):
    from nvrx_straggler import _native

    lib, st = be.lib, be.stream_handle
    for R, K, S in SHAPES:
        T = _random_table(np.random.default_rng(R * 1000 + K + S), R, K, S)
        ws = be.workspace(R, K, S, R, 0)
        ws.send.copy_(torch.from_numpy(T))
        torch.cuda.synchronize()
        out = {"what": "operator", "R": R, "K": K, "S": S, "launches": launches}

        def score():
            _native.check(lib.nvrx_score(ws.send_ptr, R, K, S, 1, 1, None, ws.d_scores, ws.d_flags, ws.d_meta, ws.d_counter, 1, None, None, 0, st))

        out["score_us"] = round(_timed(score, launches, warmup, be.stream), 2)
        for n in (5, 16):
            buf, scratch = ws.attr_buffers(R, n, True)

            def attribute():
                _native.check(lib.nvrx_attribute(ws.send_ptr, R, K, S, 0, R, n, 1, 1, scratch.data_ptr(), buf.data_ptr(), st))

            out[f"attribute_n{n}_us"] = round(_timed(attribute, launches, warmup, be.stream), 2)
        out["ratio_n5"] = round(out["attribute_n5_us"] / out["score_us"], 2)
        print(json.dumps(out), flush=True)


def report_cost(be, reports, warmup):
    from nvrx_straggler import _native
    from nvrx_straggler.reporting import ReportGenerator

    local_ranks, n_k, n_s, samples = 8, 32, 32, 10_000
    rings = be.make_rings(local_ranks, n_k + n_s, samples)
    krows = {f"kernel_{i:02d}_blk_256_1_1_grid_64_1_1": rings.row_for(_native.KIND_KERNEL, f"kernel_{i:02d}_blk_256_1_1_grid_64_1_1")
             for i in range(n_k)}
    srows = {f"section_{i:02d}": rings.row_for(_native.KIND_SECTION, f"section_{i:02d}") for i in range(n_s)}
    rng = np.random.default_rng(0)
    for lr in range(local_ranks):
        data = rng.lognormal(1.0 + 0.05 * lr, 0.2, (n_k + n_s, samples)).astype(np.float32)
        rings.push_device_rows(0, torch.from_numpy(data).to(be.device), lr=lr)
    be.synchronize()
    torch.cuda.synchronize()
    gens = {0: ReportGenerator(["relative_perf_scores", "individual_perf_scores"], node_name="n"),
            5: ReportGenerator(["relative_perf_scores", "individual_perf_scores"], node_name="n", kernel_attribution=5)}
    lat = {0: [], 5: []}
    readable = []
    try:
        for i in range(2 * (reports + warmup)):
            n = 5 if i & 1 else 0
            rings.set_count_all(samples)
            t0 = time.perf_counter_ns()
            rep = gens[n].generate_report_from_rings(rings, srows, krows, local_ranks=local_ranks)
            rep.identify_stragglers()
            t1 = time.perf_counter_ns()
            if n:
                ex = rep.explain_gpu_scores()
                t2 = time.perf_counter_ns()
                assert len(ex["relative"]) == local_ranks
            if i >= 2 * warmup:
                lat[n].append((t1 - t0) * 1e-3)
                if n:
                    readable.append((t2 - t0) * 1e-3)
            be.synchronize()
        out = {"what": "ring report, call -> flagged set", "reports_each": reports, "shape": "8 x (32 + 32) x 10000"}
        for n, key in ((0, "off"), (5, "on_n5")):
            out[f"{key}_median_us"] = round(float(np.median(lat[n])), 1)
            out[f"{key}_p95_us"] = round(float(np.percentile(lat[n], 95)), 1)
        out["delta_median_us"] = round(out["on_n5_median_us"] - out["off_median_us"], 1)
        out["attribution_readable_median_us"] = round(float(np.median(readable)), 1)
        out["attribution_readable_p95_us"] = round(float(np.percentile(readable, 95)), 1)
        # a report whose attribution nobody reads: the NEXT report on the same buffers waits for its kernel and copies the
        # records out before it rewrites the table (Workspace.attr_settle), so that cost moves into the next call
        unread = []
        for i in range(reports + warmup):
            rings.set_count_all(samples)
            t0 = time.perf_counter_ns()
            gens[5].generate_report_from_rings(rings, srows, krows, local_ranks=local_ranks).identify_stragglers()
            if i >= warmup:
                unread.append((time.perf_counter_ns() - t0) * 1e-3)
        be.synchronize()
        out["on_n5_never_read_median_us"] = round(float(np.median(unread)), 1)
        out["on_n5_never_read_p95_us"] = round(float(np.percentile(unread, 95)), 1)
        print(json.dumps(out), flush=True)
    finally:
        for g in gens.values():
            g.close()
        rings.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reports", type=int, default=200)
    args = ap.parse_args()
    from nvrx_straggler.backend import get_backend

    torch.cuda.set_device(0)
    be = get_backend()
    operator_cost(be, args.launches, args.warmup)
    report_cost(be, args.reports, args.warmup)


if __name__ == "__main__":
    main()
