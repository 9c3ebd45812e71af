#!/usr/bin/env python3
"""What work groups cost (docs/MEASUREMENTS.md, "Work groups").  One GPU:

    python tools/work_cost.py kernels [--launches 200] [--warmup 20] [--shape N]
    python tools/work_cost.py report  [--reports 200] [--warmup 20]

``kernels``: ``nvrx_work_groups`` (``k_work_sig``, ``k_work_pairs``, ``k_work_groups``, ``k_work_rank``) on tables of 8 ranks x
    (0 + 64) ids, 64 ranks x (4096 + 0) ids, 1024 ranks x (64 + 64) ids and 4096 ranks x (64 + 64) ids, the ranks in stages of
    R / 2 (R / 8 from 1024 ranks on) that differ in a tenth of their columns, ``--launches`` each after ``--warmup``, next to
    ``nvrx_peer_score`` with those stages as groups on the same tables in the same run.  Prints hipEvent microseconds per call
    (back-to-back: throughput, not latency); for per-kernel durations run it under the profiler, alone:
    ``rocprofv3 --kernel-trace --stats -d <dir> -- python tools/work_cost.py kernels --shape N`` (a run per shape: the
    kernels have one name at every size).
``report``: ``generate_report_from_rings`` + ``identify_stragglers()`` of the headline shape (8 folded ranks x 64 sections x
    10 000 samples), alternating in one process, median and p95 of ``--reports`` each: ``work_groups`` off against on, and
    ``peer_groups="block:4"`` against ``peer_groups="auto"`` (which waits for the step inside the report).
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

SHAPES = [(8, 0, 64, 2), (64, 4096, 0, 2), (1024, 64, 64, 8), (4096, 64, 64, 8)]  # (ranks, kernel ids, section ids, stages)


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


def _table(rng, R, K, S, G):
    """Stages of R / G ranks: every stage lacks its own tenth of the columns, and runs its kernels (1 + stage) x 100 times."""
    KS = K + S
    stage = np.arange(R) // (R // G)
    T = np.zeros((R, 2 * KS + K + 1), dtype=np.float32)
    med = rng.lognormal(np.log(1000.0), 0.05, (R, KS)).astype(np.float32)
    lacks = (np.arange(KS)[None, :] * 10 // max(KS, 1)) == (stage[:, None] % 10)
    med[lacks] = -1.0
    T[:, :KS] = med
    T[:, KS : 2 * KS] = np.where(med >= 0, med * 0.9, np.nan)
    T[:, 2 * KS : 2 * KS + K] = np.where(med[:, :K] >= 0, med[:, :K] * 100.0 * (1 + stage[:, None]), 0.0)
    T[:, -1] = 1.0
    return T


def kernels(args):
    from nvrx_straggler import _native
    from nvrx_straggler.backend import PeerGroups, get_backend

    torch.cuda.set_device(0)
    be = get_backend()
    lib, st = be.lib, be.stream_handle
    rng = np.random.default_rng(0)
    for n, (R, K, S, G) in enumerate(SHAPES):
        if args.shape >= 0 and n != args.shape:
            continue
        ws = be.workspace(R, K, S, R, 0)
        with torch.cuda.stream(be.stream):
            ws.send.copy_(torch.from_numpy(_table(rng, R, K, S, G)))
        groups = PeerGroups([r // (R // G) for r in range(R)])
        d_groups = groups.device(be)
        pbuf, wbuf = ws.peer_buffers(G, R), ws.work_buffers()
        be.synchronize()

        def peer():
            _native.check(lib.nvrx_peer_score(ws.send_ptr, R, K, S, d_groups.data_ptr(), G, 0, R, 2, pbuf.data_ptr(), st))

        def work():
            _native.check(lib.nvrx_work_groups(ws.send_ptr, R, K, S, 0.25, 100000, wbuf.data_ptr(), st))

        out = {"what": "kernels", "ranks": R, "kernel_ids": K, "section_ids": S, "stages": G, "launches": args.launches}
        out["peer_us"] = round(_timed(peer, args.launches, args.warmup, be.stream), 2)
        be.synchronize()
        out["work_us"] = round(_timed(work, args.launches, args.warmup, be.stream), 2)
        be.synchronize()
        _, _, rank, job, words = _native.work_offsets(R, K, S)
        out["groups_found"] = int(wbuf[job].item())
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
    for title, off_kw, on_kw in (("work_groups off / on", {}, {"work_groups": True}),
                                 ("peer_groups block:4 / auto", {"peer_groups": "block:4"}, {"peer_groups": "auto"})):
        gens = {0: ReportGenerator(["relative_perf_scores"], node_name="n", **off_kw),
                1: ReportGenerator(["relative_perf_scores"], node_name="n", **on_kw)}
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
                    assert rep.work_groups()["groups"] == {0: list(range(local_ranks))}  # (sections only, all present: one group)
                t2 = time.perf_counter_ns()
                if i >= 2 * args.warmup:
                    lat[on].append((t1 - t0) * 1e-3)
                    if on:
                        readable.append((t2 - t0) * 1e-3)
                be.synchronize()
            out = {"what": "ring report, call -> flagged set", "compared": title, "processes": 1, "reports_each": args.reports,
                   "shape": "8 x 64 x 10000"}
            for on, key in ((0, "off"), (1, "on")):
                out[f"{key}_median_us"] = round(float(np.median(lat[on])), 1)
                out[f"{key}_p95_us"] = round(float(np.percentile(lat[on], 95)), 1)
            out["delta_median_us"] = round(out["on_median_us"] - out["off_median_us"], 1)
            out["work_readable_median_us"] = round(float(np.median(readable)), 1)
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
    args = ap.parse_args()
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    {"kernels": kernels, "report": report}[args.what](args)


if __name__ == "__main__":
    main()
