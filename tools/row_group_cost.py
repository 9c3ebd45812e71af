#!/usr/bin/env python3
"""What row-family scores per peer group cost (docs/MEASUREMENTS.md, "Row-family scores per peer group").  One GPU:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/row_group_cost.py kernels --ranks 8 --ids 64 --groups 2
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/row_group_cost.py kernels --ranks 8 --ids 4096 --groups 2
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/row_group_cost.py kernels --ranks 1024 --ids 128 --groups 8
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/row_group_cost.py kernels --ranks 1024 --ids 128 --groups 128
    python tools/row_group_cost.py report [--reports 200] [--warmup 20]

``kernels``: ``--launches`` rounds of the job-wide score step (``nvrx_tail_score``: ``k_colmin``, or ``k_colmin_part`` and
    ``k_colmin_finish`` beyond 64 ranks, then ``k_tail_score``) and of the step per peer group (``nvrx_rowfam_group_score``:
    ``k_peer_cols``, ``k_rowfam_group_rank``) on the SAME tail table of ``--ranks`` ranks x ``--ids`` ids (half kernels, half
    sections; all of them sections at 64 ids) in ``--groups`` equal groups (``block`` labels), alternating on one stream.  Meant
    to run under ``rocprofv3 --kernel-trace --stats``, whose statistics give each kernel's time, one shape per run; by itself
    it prints the hipEvent time of a round of each step (kernels back to back: throughput, not latency), each taken twice so
    that the spread of a step against itself is on the page.
``report``: a synchronous ring report of 8 folded ranks x 64 sections x 10 000 samples with ``tail_quantile=0.95`` and
    ``peer_groups="block:4"`` set and ``row_peer_groups`` on and off alternating in one process; median and p95 of
    ``--reports`` each, and the time until ``identify_tail_stragglers()`` has returned.
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


def kernels(args):
    from nvrx_straggler import _native
    from nvrx_straggler.backend import PeerGroups, get_backend

    torch.cuda.set_device(0)
    be = get_backend()
    lib, st = be.lib, be._stream_handle
    rng = np.random.default_rng(0)
    R, G = args.ranks, args.groups
    K, S = (0, args.ids) if args.ids <= 64 else (args.ids // 2, args.ids - args.ids // 2)
    KS = K + S
    if R % G:
        raise SystemExit("--ranks must be a multiple of --groups")
    groups = PeerGroups([r // (R // G) for r in range(R)])
    T = np.zeros((R, _native.table_len(K, S)), dtype=np.float32)
    T[:, 2 * KS: 2 * KS + K] = rng.uniform(1e3, 1e5, (R, K))
    with torch.cuda.stream(be.stream):
        tails = torch.from_numpy(rng.lognormal(7.0, 0.05, (R, KS)).astype(np.float32)).to(be.device)
        table = torch.from_numpy(T).to(be.device)
        scratch = torch.empty(max(33 * KS, 64), dtype=torch.float32, device=be.device)
        wide = torch.empty(R * (1 + S), dtype=torch.float32, device=be.device)
        grouped = torch.empty(_native.rowfam_group_words(G, K, S, R), dtype=torch.float32, device=be.device)
    d_groups = groups.device(be)
    be.synchronize()

    def job_wide():
        _native.check(lib.nvrx_tail_score(tails.data_ptr(), table.data_ptr(), R, K, S, 0, R, scratch.data_ptr(), wide.data_ptr(), st))

    def per_group():
        _native.check(lib.nvrx_rowfam_group_score(tails.data_ptr(), 1, table.data_ptr(), R, K, S, d_groups.data_ptr(), G, 0, R, 2,
                                                  grouped.data_ptr(), st))

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
    print(json.dumps({"what": "kernels", "ranks": R, "kernel_ids": K, "section_ids": S, "groups": G, "launches": args.launches,
                      "job_wide_round_us": rounds["job_wide"], "per_group_round_us": rounds["per_group"]}), flush=True)


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
    common = dict(node_name="n", tail_quantile=0.95, peer_groups="block:4")
    gens = {"off": ReportGenerator(["relative_perf_scores"], **common),
            "on": ReportGenerator(["relative_perf_scores"], row_peer_groups=True, **common)}
    lat, readable = {"off": [], "on": []}, {"off": [], "on": []}
    order = ("off", "on", "on", "off")  # each configuration follows itself and the other
    try:
        for i in range(2 * (args.reports + args.warmup)):
            key = order[i % 4]
            rings.set_count_all(samples)
            t0 = time.perf_counter_ns()
            rep = gens[key].generate_report_from_rings(rings, srows, {}, local_ranks=local_ranks)
            rep.identify_stragglers()
            t1 = time.perf_counter_ns()
            rep.identify_tail_stragglers()
            t2 = time.perf_counter_ns()
            if i >= 2 * args.warmup:
                lat[key].append((t1 - t0) * 1e-3)
                readable[key].append((t2 - t0) * 1e-3)
            be.synchronize()
        out = {"what": "ring report with tail_quantile and peer_groups, call -> flagged set", "processes": 1,
               "reports_each": args.reports, "shape": "8 x 64 sections x 10000", "peer_groups": "block:4"}
        for key in ("off", "on"):
            out[f"{key}_median_us"] = round(float(np.median(lat[key])), 1)
            out[f"{key}_p95_us"] = round(float(np.percentile(lat[key], 95)), 1)
            out[f"{key}_tails_readable_median_us"] = round(float(np.median(readable[key])), 1)
        out["delta_median_us"] = round(out["on_median_us"] - out["off_median_us"], 1)
        out["delta_tails_readable_median_us"] = round(out["on_tails_readable_median_us"] - out["off_tails_readable_median_us"], 1)
        print(json.dumps(out), flush=True)
    finally:
        for g in gens.values():
            g.close()
        rings.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "report"])
    ap.add_argument("--ranks", type=int, default=8)
    ap.add_argument("--ids", type=int, default=64)
    ap.add_argument("--groups", type=int, default=2)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reports", type=int, default=200)
    args = ap.parse_args()
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    {"kernels": kernels, "report": report}[args.what](args)


if __name__ == "__main__":
    main()
