#!/usr/bin/env python3
"""What slack scores per peer group cost (docs/MEASUREMENTS.md, "Slack scores per peer group").  One GPU:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/slack_group_cost.py kernels-group --ranks 8 --groups 2
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/slack_group_cost.py kernels-group --ranks 1024 --groups 128
    python tools/slack_group_cost.py report [--reports 200] [--warmup 20]

``kernels-group``: ``--launches`` rounds of the job-wide score step (``nvrx_slack_score``: ``k_slack_cols``, ``k_slack_rank``,
    ``k_slack_job``) and of the step per peer group (``nvrx_slack_group_score``: ``k_slack_group_cols``, ``k_slack_rank<true>``,
    ``k_slack_group_job``) on the SAME gathered table of ``--ranks`` ranks in ``--groups`` equal groups (``block`` labels) with
    24 columns in use and 64 kernel ids, alternating on one stream.  Meant to run under ``rocprofv3 --kernel-trace --stats``,
    whose statistics give each kernel's time, one shape per run; by itself it prints the hipEvent time of a round of each step
    (three kernels back to back: throughput, not latency), each taken twice so that the spread of a step against itself is
    on the page.
``report``: ``tools/slack_cost.py report``'s shape with ``collective_slack`` and ``peer_groups="block:4"`` set and
    ``slack_peer_groups`` on and off alternating in one process; median and p95 of ``--reports`` each, and the time until
    ``identify_slack_stragglers()`` has returned.
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


def kernels_group(args):
    from nvrx_straggler import _native
    from nvrx_straggler.backend import PeerGroups, get_backend
    from nvrx_straggler.reporting import slack_column

    torch.cuda.set_device(0)
    be = get_backend()
    lib, st = be.lib, be._stream_handle
    rng = np.random.default_rng(0)
    R, G, K, S = args.ranks, args.groups, 64, 64
    if R % G:
        raise SystemExit("--ranks must be a multiple of --groups")
    groups = PeerGroups([r // (R // G) for r in range(R)])
    ws = be.workspace(R, K, S, R, 0)
    _, table, out = ws.slack_buffers(_native.slack_group_words(G, R))
    slack = np.zeros((R, 2, _native.SLACK_COLS), dtype=np.float32)
    slack[:, 0, :] = -1.0
    used = sorted({slack_column(k) for k in COLLECTIVES})
    calls = rng.integers(100, 300, (R, len(used))).astype(np.float32)
    slack[:, 1, used] = calls
    slack[:, 0, used] = calls * rng.lognormal(5.3, 0.1, (R, len(used))).astype(np.float32)
    with torch.cuda.stream(be.stream):
        table.copy_(torch.from_numpy(slack.reshape(R, -1)))
        T = np.zeros((R, _native.table_len(K, S)), dtype=np.float32)
        T[:, 2 * (K + S): 2 * (K + S) + K] = rng.uniform(1e3, 1e5, (R, K))
        ws.send.copy_(torch.from_numpy(T))
    d_groups = groups.device(be)
    be.synchronize()

    def job_wide():
        _native.check(lib.nvrx_slack_score(table.data_ptr(), ws.send_ptr, R, K, S, min(4, R), out.data_ptr(), st))

    def per_group():
        _native.check(lib.nvrx_slack_group_score(table.data_ptr(), ws.send_ptr, R, K, S, d_groups.data_ptr(), G, groups.max_size, 4,
                                                 2, out.data_ptr(), st))

    for _ in range(args.warmup):
        job_wide()
        per_group()
    be.synchronize()
    rounds = {"job_wide": [], "per_group": []}
    for name, fn in (("job_wide", job_wide), ("per_group", per_group)) * 2:  # alternating, each twice
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(be.stream)
        for _ in range(args.launches):
            fn()
        t1.record(be.stream)
        t1.synchronize()
        rounds[name].append(round(t0.elapsed_time(t1) * 1e3 / args.launches, 2))
    print(json.dumps({"what": "kernels-group", "ranks": R, "groups": G, "max_group": groups.max_size, "kernel_ids": K,
                      "columns_in_use": len(used), "launches": args.launches, "job_wide_round_us": rounds["job_wide"],
                      "per_group_round_us": rounds["per_group"]}), flush=True)


def report(args):
    torch.cuda.set_device(0)
    from nvrx_straggler import _native
    from nvrx_straggler.backend import get_backend
    from nvrx_straggler.reporting import ReportGenerator

    be = get_backend()
    local_ranks, sections, samples = 8, 64, 10_000
    rings = be.make_rings(local_ranks, sections + 1 + len(COLLECTIVES), samples)
    srows = {f"section_{i:03d}": rings.row_for(_native.KIND_SECTION, f"section_{i:03d}") for i in range(sections)}
    krows = {"gemm": rings.row_for(_native.KIND_KERNEL, "gemm")}  # (the planned, one-call path: tools/slack_cost.py)
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
    common = dict(node_name="n", collective_slack=True, peer_groups="block:4")
    gens = {"off": ReportGenerator(["relative_perf_scores"], **common),
            "on": ReportGenerator(["relative_perf_scores"], slack_peer_groups=True, **common)}
    lat, readable = {"off": [], "on": []}, {"off": [], "on": []}
    order = ("off", "on", "on", "off")  # each configuration follows itself and the other
    try:
        for i in range(2 * (args.reports + args.warmup)):
            key = order[i % 4]
            rings.set_count_all(samples)
            t0 = time.perf_counter_ns()
            rep = gens[key].generate_report_from_rings(rings, srows, krows, local_ranks=local_ranks)
            rep.identify_stragglers()
            t1 = time.perf_counter_ns()
            rep.identify_slack_stragglers()
            t2 = time.perf_counter_ns()
            if i >= 2 * args.warmup:
                lat[key].append((t1 - t0) * 1e-3)
                readable[key].append((t2 - t0) * 1e-3)
            be.synchronize()
        out = {"what": "ring report with collective_slack and peer_groups, call -> flagged set", "processes": 1,
               "reports_each": args.reports, "shape": "8 x (64 sections + 25 kernel rows) x 10000", "peer_groups": "block:4"}
        for key in ("off", "on"):
            out[f"{key}_median_us"] = round(float(np.median(lat[key])), 1)
            out[f"{key}_p95_us"] = round(float(np.percentile(lat[key], 95)), 1)
            out[f"{key}_slack_readable_median_us"] = round(float(np.median(readable[key])), 1)
        out["delta_median_us"] = round(out["on_median_us"] - out["off_median_us"], 1)
        print(json.dumps(out), flush=True)
    finally:
        for g in gens.values():
            g.close()
        rings.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels-group", "report"])
    ap.add_argument("--ranks", type=int, default=8)
    ap.add_argument("--groups", type=int, default=2)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reports", type=int, default=200)
    args = ap.parse_args()
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    {"kernels-group": kernels_group, "report": report}[args.what](args)


if __name__ == "__main__":
    main()
