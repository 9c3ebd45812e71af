#!/usr/bin/env python3
"""What pace scores cost (docs/MEASUREMENTS.md, "Pace scores").  One GPU:

    python tools/pace_cost.py kernels [--launches 200] [--warmup 20]
    python tools/pace_cost.py report  [--reports 200] [--warmup 20]

``kernels``: ``nvrx_pace_score`` (``k_pace_cols`` + ``k_pace_rank``, every rank reported) on random tables of 8 ranks x
    (0 + 64) ids, 8 ranks x (4096 + 0) ids and 1024 ranks x (64 + 64) ids, ``--launches`` each after ``--warmup``, next to
    ``nvrx_robust_score`` on the same tables in the same run.  Prints hipEvent microseconds per call of the pair
    (back-to-back: throughput, not latency); for the duration of each of the two launches run it under the profiler, alone:
    ``rocprofv3 --kernel-trace --stats -d <dir> -- python tools/pace_cost.py kernels --shape N`` (a run per shape).
``report``: ``generate_report_from_rings`` + ``identify_stragglers()`` of the headline shape (8 folded ranks x 64 sections x
    10 000 samples) with ``pace_scores`` off and on, alternating in one process, median and p95 of ``--reports`` each; with
    the option on also the time until ``pace_scores()`` has returned.
``--grouped``: pace scores per peer group (docs/MEASUREMENTS.md, "Pace scores per peer group").  ``kernels``:
    ``nvrx_pace_group_score`` (``k_pace_group_cols`` + the grouped ``k_pace_rank``) next to ``nvrx_pace_score`` on the same
    tables in the same run: 8 ranks x 64 sections in 2 groups, 8 ranks x 4096 kernels in 2 groups, 1024 ranks x 128 ids in 8
    and in 128 groups (``mod:G``: interleaved memberships); under the profiler a run per ``--shape``.  ``report``: both
    generators have ``pace_scores`` and ``peer_groups="mod:2"``, ``pace_peer_groups`` is what alternates.
``--node``: node scores (docs/MEASUREMENTS.md, "Node scores").  ``kernels``: ``nvrx_node_score`` (``k_node_cols``, or
    ``k_pace_group_cols`` + ``k_node_across``, then the rank kernel twice) next to ``nvrx_pace_score`` and
    ``nvrx_pace_group_score`` on the same tables in the same run: 8 ranks x 64 sections on 2 nodes, 64 ranks x 4096 kernels
    on 8 nodes, 1024 ranks x 128 ids on 128 nodes (``block:N``); under the profiler a run per ``--shape``.  ``report``:
    ``node_scores`` (``node_groups="block:4"``) is what alternates.
``--families`` (``report`` only; docs/MEASUREMENTS.md, "Table families"): ``robust_scores``, ``pace_scores`` and ``node_scores``
    (``node_groups="block:4"``) all on is what alternates with a plain generator.
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

SHAPES = [(8, 0, 64), (8, 4096, 0), (1024, 64, 64)]  # (ranks, kernel ids, section ids)
NODE_SHAPES = [(8, 0, 64, 2), (64, 4096, 0, 8), (1024, 64, 64, 128)]  # (..., nodes)
GROUPED_SHAPES = [(8, 0, 64, 2), (8, 4096, 0, 2), (1024, 64, 64, 8), (1024, 64, 64, 128)]  # (..., groups)


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


def _table(rng, R, K, S):
    KS = K + S
    T = np.zeros((R, 2 * KS + K + 1), dtype=np.float32)
    med = rng.lognormal(np.log(1000.0), 0.05, (R, KS)).astype(np.float32)
    med[rng.random((R, KS)) < 0.05] = -1.0
    T[:, :KS] = med
    T[:, KS : 2 * KS] = np.where(med >= 0, med * 0.9, np.nan)
    T[:, 2 * KS : 2 * KS + K] = np.where(med[:, :K] >= 0, rng.uniform(1, 1000, (R, K)), 0.0)
    T[:, -1] = 1.0
    return T


def kernels(args):
    from nvrx_straggler import _native
    from nvrx_straggler.backend import get_backend

    torch.cuda.set_device(0)
    be = get_backend()
    lib, st = be.lib, be.stream_handle
    rng = np.random.default_rng(0)
    for i, (R, K, S) in enumerate(SHAPES):
        if args.shape >= 0 and i != args.shape:
            continue
        ws = be.workspace(R, K, S, R, 0)
        with torch.cuda.stream(be.stream):
            ws.send.copy_(torch.from_numpy(_table(rng, R, K, S)))
        rbuf, pbuf = ws.robust_buffers(R), ws.pace_buffers(R)
        be.synchronize()

        def robust():
            _native.check(lib.nvrx_robust_score(ws.send_ptr, R, K, S, 0, R, 4, 0.02, rbuf.data_ptr(), st))

        def pace():
            _native.check(lib.nvrx_pace_score(ws.send_ptr, R, K, S, 0, R, 4, pbuf.data_ptr(), st))

        out = {"what": "kernels", "ranks": R, "kernel_ids": K, "section_ids": S, "launches": args.launches}
        out["robust_us"] = round(_timed(robust, args.launches, args.warmup, be.stream), 2)
        be.synchronize()
        out["pace_us"] = round(_timed(pace, args.launches, args.warmup, be.stream), 2)
        print(json.dumps(out), flush=True)


def kernels_grouped(args):
    from nvrx_straggler import _native
    from nvrx_straggler.backend import PeerGroups, get_backend

    torch.cuda.set_device(0)
    be = get_backend()
    lib, st = be.lib, be.stream_handle
    rng = np.random.default_rng(0)
    for i, (R, K, S, G) in enumerate(GROUPED_SHAPES):
        if args.shape >= 0 and i != args.shape:
            continue
        ws = be.workspace(R, K, S, R, 0)
        with torch.cuda.stream(be.stream):
            ws.send.copy_(torch.from_numpy(_table(rng, R, K, S)))
        groups = PeerGroups([r % G for r in range(R)])
        pbuf = ws.pace_buffers(R, G)
        gptr, largest = groups.device(be).data_ptr(), groups.max_size
        be.synchronize()

        def pace():
            _native.check(lib.nvrx_pace_score(ws.send_ptr, R, K, S, 0, R, 4, pbuf.data_ptr(), st))

        def grouped():
            _native.check(lib.nvrx_pace_group_score(ws.send_ptr, R, K, S, gptr, G, largest, 0, R, 4, 2, pbuf.data_ptr(), st))

        out = {"what": "kernels, grouped", "ranks": R, "kernel_ids": K, "section_ids": S, "groups": G, "largest": largest,
               "launches": args.launches}
        out["pace_us"] = round(_timed(pace, args.launches, args.warmup, be.stream), 2)
        be.synchronize()
        out["pace_group_us"] = round(_timed(grouped, args.launches, args.warmup, be.stream), 2)
        print(json.dumps(out), flush=True)


def kernels_node(args):
    from nvrx_straggler import _native
    from nvrx_straggler.backend import PeerGroups, get_backend

    torch.cuda.set_device(0)
    be = get_backend()
    lib, st = be.lib, be.stream_handle
    rng = np.random.default_rng(0)
    for i, (R, K, S, G) in enumerate(NODE_SHAPES):
        if args.shape >= 0 and i != args.shape:
            continue
        ws = be.workspace(R, K, S, R, 0)
        with torch.cuda.stream(be.stream):
            ws.send.copy_(torch.from_numpy(_table(rng, R, K, S)))
        nodes = PeerGroups([r // (R // G) for r in range(R)])
        pbuf, nbuf = ws.pace_buffers(R, G), ws.node_buffers(G, R)
        gptr, largest = nodes.device(be).data_ptr(), nodes.max_size
        be.synchronize()

        def pace():
            _native.check(lib.nvrx_pace_score(ws.send_ptr, R, K, S, 0, R, 4, pbuf.data_ptr(), st))

        def grouped():
            _native.check(lib.nvrx_pace_group_score(ws.send_ptr, R, K, S, gptr, G, largest, 0, R, 2, 1, pbuf.data_ptr(), st))

        def node():
            _native.check(lib.nvrx_node_score(ws.send_ptr, R, K, S, gptr, G, largest, 2, min(3, G), 0, R, nbuf.data_ptr(), st))

        out = {"what": "kernels, node", "ranks": R, "kernel_ids": K, "section_ids": S, "nodes": G, "largest": largest,
               "launches": args.launches}
        for name, fn in (("pace_us", pace), ("pace_group_us", grouped), ("node_us", node)):
            out[name] = round(_timed(fn, args.launches, args.warmup, be.stream), 2)
            be.synchronize()
        print(json.dumps(out), flush=True)


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
            1: ReportGenerator(["relative_perf_scores"], node_name="n", pace_scores=True)}
    if args.grouped:
        gens = {0: ReportGenerator(["relative_perf_scores"], node_name="n", pace_scores=True, peer_groups="mod:2"),
                1: ReportGenerator(["relative_perf_scores"], node_name="n", pace_scores=True, peer_groups="mod:2",
                                   pace_peer_groups=True)}
    if args.node:
        gens = {0: ReportGenerator(["relative_perf_scores"], node_name="n"),
                1: ReportGenerator(["relative_perf_scores"], node_name="n", node_scores=True, node_groups="block:4")}
    if args.families:
        gens = {0: ReportGenerator(["relative_perf_scores"], node_name="n"),
                1: ReportGenerator(["relative_perf_scores"], node_name="n", robust_scores=True, pace_scores=True,
                                   node_scores=True, node_groups="block:4")}
    lat, readable = {0: [], 1: []}, []
    try:
        for i in range(2 * (args.reports + args.warmup)):
            on = (i & 1) ^ ((i >> 1) & 1)  # off on on off ...
            rings.set_count_all(samples)
            t0 = time.perf_counter_ns()
            rep = gens[on].generate_report_from_rings(rings, srows, krows, local_ranks=local_ranks)
            rep.identify_stragglers()
            t1 = time.perf_counter_ns()
            if on:
                scores = rep.node_scores() if args.node or args.families else rep.pace_scores()
                assert len(scores["section_columns"]) == sections
                if args.families:
                    assert rep.robust_scores() and rep.pace_scores()
            t2 = time.perf_counter_ns()
            if i >= 2 * args.warmup:
                lat[on].append((t1 - t0) * 1e-3)
                if on:
                    readable.append((t2 - t0) * 1e-3)
            be.synchronize()
        out = {"what": "ring report, call -> flagged set" + (", pace_peer_groups off / on" if args.grouped else ", node_scores off / on" if args.node else ", robust + pace + node scores off / on" if args.families else ""), "processes": 1, "reports_each": args.reports, "shape": "8 x 64 x 10000"}
        for on, key in ((0, "off"), (1, "on")):
            out[f"{key}_median_us"] = round(float(np.median(lat[on])), 1)
            out[f"{key}_p95_us"] = round(float(np.percentile(lat[on], 95)), 1)
        out["delta_median_us"] = round(out["on_median_us"] - out["off_median_us"], 1)
        out["all_readable_median_us" if args.families else "node_readable_median_us" if args.node else "pace_readable_median_us"] = round(float(np.median(readable)), 1)
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
    ap.add_argument("--shape", type=int, default=-1, help="kernels: only that entry of SHAPES (a profiler run per shape)")
    ap.add_argument("--grouped", action="store_true", help="pace scores per peer group (see the module's text)")
    ap.add_argument("--node", action="store_true", help="node scores (see the module's text)")
    ap.add_argument("--families", action="store_true", help="report: robust, pace and node scores together (see the module's text)")
    args = ap.parse_args()
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    {"kernels": kernels_node if args.node else kernels_grouped if args.grouped else kernels, "report": report}[args.what](args)


if __name__ == "__main__":
    main()
