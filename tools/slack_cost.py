#!/usr/bin/env python3
"""What slack scores cost (docs/MEASUREMENTS.md, "Slack scores").  One GPU:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/slack_cost.py kernels --ranks 8 [--launches 200]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/slack_cost.py kernels --ranks 1024
    python tools/slack_cost.py report [--reports 200] [--warmup 20]

``kernels``: ``--launches`` rounds of the local step (``nvrx_slack_local``: ``k_slack_local`` over 8 logical ranks with 24
    collective rows each) and of the score step (``nvrx_slack_score``: ``k_slack_cols``, ``k_slack_rank``, ``k_slack_job``) on
    a gathered table of ``--ranks`` ranks with 24 columns in use and 64 kernel ids, back to back on one stream.  Meant to run
    under ``rocprofv3 --kernel-trace --stats``, whose statistics give each kernel's time; by itself it prints the hipEvent
    time of a round (all four kernels back to back: throughput, not latency).
``report``: ``generate_report_from_rings`` + ``identify_stragglers()`` of the headline shape (8 folded ranks x 64 sections x
    10 000 samples, plus one compute kernel and 24 collective kernels of 10 000 calls each per rank), synchronous, with the
    option on and off alternating in one process; median and p95 of ``--reports`` each; with the option on also the time
    until ``identify_slack_stragglers()`` has returned.
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

COLLECTIVES = [f"ncclDevKernel_Generic_{i}(ncclDevKernelArgsStorage<4096ul>)" for i in range(24)]


def kernels(args):
    from nvrx_straggler import _native
    from nvrx_straggler.backend import get_backend

    torch.cuda.set_device(0)
    be = get_backend()
    lib, st = be.lib, be._stream_handle
    rng = np.random.default_rng(0)
    R, K, S, local_ranks, rows_per_rank = args.ranks, 64, 64, 8, 128
    rings = be.make_rings(local_ranks, rows_per_rank, 64)
    try:
        for name in ["gemm"] + COLLECTIVES:
            rings.row_for(_native.KIND_KERNEL, name)
        for lr in range(local_ranks):
            for row in range(1 + len(COLLECTIVES)):
                rings.push_many(row, rng.lognormal(5.3, 0.1, 48).astype(np.float32), lr=lr)
        ws_local = be.workspace(local_ranks, 1, 0, local_ranks, local_ranks * rows_per_rank)
        rings.report_local(ws_local, True, rows_active=rings.rows_used)
        rows, cols, _ = rings.slack_list()
        ws = be.workspace(R, K, S, R, 0)
        send, table, out = ws.slack_buffers()
        local_send = torch.empty((local_ranks, 2 * _native.SLACK_COLS), dtype=torch.float32, device=be.device)
        slack = np.zeros((R, 2, _native.SLACK_COLS), dtype=np.float32)
        slack[:, 0, :] = -1.0
        used = sorted(set(cols.tolist()))
        calls = rng.integers(100, 300, (R, len(used))).astype(np.float32)
        slack[:, 1, used] = calls
        slack[:, 0, used] = calls * rng.lognormal(5.3, 0.1, (R, len(used))).astype(np.float32)
        with torch.cuda.stream(be.stream):
            table.copy_(torch.from_numpy(slack.reshape(R, -1)))
            T = np.zeros((R, _native.table_len(K, S)), dtype=np.float32)
            T[:, 2 * (K + S): 2 * (K + S) + K] = rng.uniform(1e3, 1e5, (R, K))
            ws.send.copy_(torch.from_numpy(T))
        be.synchronize()

        def one_round():
            _native.check(lib.nvrx_slack_local(rings.ctx, None, ws_local.d_stats, rows.ctypes.data, cols.ctypes.data, rows.size,
                                               local_send.data_ptr(), rings.rows_used, st))
            _native.check(lib.nvrx_slack_score(table.data_ptr(), ws.send_ptr, R, K, S, min(4, R), out.data_ptr(), st))

        for _ in range(args.warmup):
            one_round()
        be.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(be.stream)
        for _ in range(args.launches):
            one_round()
        t1.record(be.stream)
        t1.synchronize()
        print(json.dumps({"what": "kernels", "ranks": R, "kernel_ids": K, "columns_in_use": len(used), "collective_rows": int(rows.size),
                          "local_ranks": local_ranks, "launches": args.launches,
                          "round_of_four_kernels_us": round(t0.elapsed_time(t1) * 1e3 / args.launches, 2)}), flush=True)
    finally:
        rings.close()


def report(args):
    torch.cuda.set_device(0)
    from nvrx_straggler import _native
    from nvrx_straggler.backend import get_backend
    from nvrx_straggler.reporting import ReportGenerator

    be = get_backend()
    local_ranks, sections, samples = 8, 64, 10_000
    rings = be.make_rings(local_ranks, sections + 1 + len(COLLECTIVES), samples)
    srows = {f"section_{i:03d}": rings.row_for(_native.KIND_SECTION, f"section_{i:03d}") for i in range(sections)}
    # the caller's table names the compute kernel only, so that the reports take the planned, one-call path the other options'
    # figures were taken on (a table that names collective kernels is filtered at every report: the general path); the slack
    # step reads the rings' own table
    krows = {"gemm": rings.row_for(_native.KIND_KERNEL, "gemm")}
    for name in COLLECTIVES:
        rings.row_for(_native.KIND_KERNEL, name)
    rng = np.random.default_rng(0)
    for lr in range(local_ranks):
        data = rng.lognormal(np.log(1000.0), 0.02, (sections, samples)).astype(np.float32)
        rings.push_device_rows(0, torch.from_numpy(data).to(be.device), lr=lr)
        kdata = rng.lognormal(np.log(200.0), 0.02, (1 + len(COLLECTIVES), samples)).astype(np.float32)
        rings.push_device_rows(sections, torch.from_numpy(kdata).to(be.device), lr=lr)
    be.synchronize()
    torch.cuda.synchronize()
    gens = {"off": ReportGenerator(["relative_perf_scores"], node_name="n"),
            "on": ReportGenerator(["relative_perf_scores"], node_name="n", collective_slack=True)}
    lat, readable = {"off": [], "on": []}, []
    order = ("off", "on", "on", "off")  # each configuration follows itself and the other
    try:
        for i in range(2 * (args.reports + args.warmup)):
            key = order[i % 4]
            rings.set_count_all(samples)
            t0 = time.perf_counter_ns()
            rep = gens[key].generate_report_from_rings(rings, srows, krows, local_ranks=local_ranks)
            rep.identify_stragglers()
            t1 = time.perf_counter_ns()
            if key == "on":
                rep.identify_slack_stragglers()
            t2 = time.perf_counter_ns()
            if i >= 2 * args.warmup:
                lat[key].append((t1 - t0) * 1e-3)
                if key == "on":
                    readable.append((t2 - t0) * 1e-3)
            be.synchronize()
        out = {"what": "ring report, call -> flagged set", "processes": 1, "reports_each": args.reports,
               "shape": "8 x (64 sections + 25 kernel rows) x 10000", "collective_rows": len(COLLECTIVES)}
        for key in ("off", "on"):
            out[f"{key}_median_us"] = round(float(np.median(lat[key])), 1)
            out[f"{key}_p95_us"] = round(float(np.percentile(lat[key], 95)), 1)
        out["slack_delta_median_us"] = round(out["on_median_us"] - out["off_median_us"], 1)
        out["slack_readable_median_us"] = round(float(np.median(readable)), 1)
        print(json.dumps(out), flush=True)
    finally:
        for g in gens.values():
            g.close()
        rings.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "report"])
    ap.add_argument("--ranks", type=int, default=8)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reports", type=int, default=200)
    args = ap.parse_args()
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    {"kernels": kernels, "report": report}[args.what](args)


if __name__ == "__main__":
    main()
