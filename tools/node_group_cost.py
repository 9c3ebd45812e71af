#!/usr/bin/env python3
"""What node scores per peer group cost (docs/MEASUREMENTS.md, "Node scores per peer group").  One GPU:

    python tools/node_group_cost.py kernels --ranks 8 --ids 64 --per-node 2 --groups 2
    python tools/node_group_cost.py kernels --ranks 64 --ids 4096 --per-node 8 --groups 2
    python tools/node_group_cost.py kernels --ranks 1024 --ids 128 --per-node 8 --groups 8
    python tools/node_group_cost.py kernels --ranks 1024 --ids 128 --per-node 4 --groups 128
    python tools/node_group_cost.py report [--reports 200] [--warmup 20]

``kernels``: ``--launches`` rounds of the job-wide node step (``nvrx_node_score``), of the step per peer group
    (``nvrx_node_group_score``) and of ``nvrx_pace_group_score`` on the CELL array (block A's launch and one rank kernel: what
    the per-cell records alone cost in a launch of their own, next to which the fused ``k_node_group_cols`` can be read at up to
    64 ranks) on the SAME table of ``--ranks`` ranks x ``--ids`` ids (half kernels, half sections; all of them sections at 64
    ids) on nodes of ``--per-node`` ranks in ``--groups`` equal peer groups (``block`` labels both), alternating on one stream.
    It prints the hipEvent time of a round of each (kernels back to back: throughput, not latency), each taken twice so that the
    spread of a step against itself is on the page.
``report``: a synchronous ring report of 8 folded ranks x 64 sections x 10 000 samples with ``node_scores`` (``block:2``) and
    ``peer_groups="block:4"`` set and ``node_peer_groups`` on and off alternating in one process; median and p95 of
    ``--reports`` each, and the time until ``identify_node_stragglers()`` has returned.
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
    from nvrx_straggler.backend import NodeCells, PeerGroups, get_backend

    torch.cuda.set_device(0)
    be = get_backend()
    lib, st = be.lib, be._stream_handle
    R, G, P = args.ranks, args.groups, args.per_node
    K, S = (0, args.ids) if args.ids <= 64 else (args.ids // 2, args.ids - args.ids // 2)
    if R % G or R % P:
        raise SystemExit("--ranks must be a multiple of --groups and of --per-node")
    nodes, peers = PeerGroups([r // P for r in range(R)]), PeerGroups([r // (R // G) for r in range(R)])
    cells = NodeCells(nodes, peers)
    C = cells.G[0]
    rng, KS = np.random.default_rng(0), K + S
    T = np.zeros((R, _native.table_len(K, S)), dtype=np.float32)
    T[:, :KS] = np.where(rng.random((R, KS)) < 0.15, -1.0, rng.lognormal(1.0, 0.5, (R, KS)))  # 15 % of the entries absent
    T[:, 2 * KS: 2 * KS + K] = rng.uniform(1e3, 1e5, (R, K))
    with torch.cuda.stream(be.stream):
        table = torch.from_numpy(T).to(be.device)
        wide = torch.empty(_native.node_words(nodes.G, R, K, S), dtype=torch.int32, device=be.device)
        grouped = torch.empty(_native.node_group_words(*cells.G, R, K, S), dtype=torch.int32, device=be.device)
        alone = torch.empty(_native.pace_group_words(C, R, K, S), dtype=torch.int32, device=be.device)
    d_nodes, d_cells = nodes.device(be), cells.device(be)
    be.synchronize()
    min_nodes = min(3, nodes.G)

    def job_wide():
        _native.check(lib.nvrx_node_score(table.data_ptr(), R, K, S, d_nodes.data_ptr(), nodes.G, nodes.max_size, 2, min_nodes, 0, R,
                                          wide.data_ptr(), st))

    def per_group():
        _native.check(lib.nvrx_node_group_score(table.data_ptr(), R, K, S, d_cells.data_ptr(), *cells.G, *cells.maxima, 2, min_nodes, 2,
                                                0, R, grouped.data_ptr(), st))

    def cells_alone():
        _native.check(lib.nvrx_pace_group_score(table.data_ptr(), R, K, S, d_cells.data_ptr(), C, cells.maxima[0], 0, R, 2, 1,
                                                alone.data_ptr(), st))

    steps = [("job_wide", job_wide), ("per_group", per_group), ("cells_pace_group", cells_alone)]
    for _ in range(args.warmup):
        for _, fn in steps:
            fn()
    be.synchronize()
    rounds = {name: [] for name, _ in steps}
    for name, fn in steps * 2:  # alternating, each twice
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(be.stream)
        for _ in range(args.launches):
            fn()
        t1.record(be.stream)
        t1.synchronize()
        rounds[name].append(round(t0.elapsed_time(t1) * 1e3 / args.launches, 2))
    print(json.dumps({"what": "kernels", "ranks": R, "kernel_ids": K, "section_ids": S, "nodes": nodes.G, "groups": G, "cells": C,
                      "maxima": cells.maxima, "launches": args.launches, **{name + "_round_us": v for name, v in rounds.items()}}),
          flush=True)


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
    common = dict(node_name="n", node_scores=True, node_groups="block:2", peer_groups="block:4")
    gens = {"off": ReportGenerator(["relative_perf_scores"], **common),
            "on": ReportGenerator(["relative_perf_scores"], node_peer_groups=True, **common)}
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
            rep.identify_node_stragglers()
            t2 = time.perf_counter_ns()
            if i >= 2 * args.warmup:
                lat[key].append((t1 - t0) * 1e-3)
                readable[key].append((t2 - t0) * 1e-3)
            be.synchronize()
        out = {"what": "ring report with node_scores and peer_groups, call -> flagged set", "processes": 1,
               "reports_each": args.reports, "shape": "8 x 64 sections x 10000", "node_groups": "block:2", "peer_groups": "block:4"}
        for key in ("off", "on"):
            out[f"{key}_median_us"] = round(float(np.median(lat[key])), 1)
            out[f"{key}_p95_us"] = round(float(np.percentile(lat[key], 95)), 1)
            out[f"{key}_node_readable_median_us"] = round(float(np.median(readable[key])), 1)
        out["delta_median_us"] = round(out["on_median_us"] - out["off_median_us"], 1)
        out["delta_node_readable_median_us"] = round(out["on_node_readable_median_us"] - out["off_node_readable_median_us"], 1)
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
    ap.add_argument("--per-node", type=int, default=2)
    ap.add_argument("--groups", type=int, default=2)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reports", type=int, default=200)
    args = ap.parse_args()
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    {"kernels": kernels, "report": report}[args.what](args)


if __name__ == "__main__":
    main()
