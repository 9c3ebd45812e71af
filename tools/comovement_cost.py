#!/usr/bin/env python3
"""What the co-movement groups cost (docs/MEASUREMENTS.md, "Co-movement groups").  One GPU:

    python tools/comovement_cost.py round  [--launches 50] [--warmup 5] [--repeats 5]
    python tools/comovement_cost.py pairs  [--launches 50]
    python tools/comovement_cost.py report [--reports 50] [--warmup 5]

``round``: ``nvrx_comove_groups`` (centre, unit timelines, pairs, components, records: six launches) at 8 ranks x B 32 and at
    1024 and 4096 ranks x B 64, next to ``nvrx_work_groups`` at the same R (K + S = 128 columns) in the same run, alternating
    -- a yardstick, not a threshold.  Half the ranks follow one of 16 planted patterns.  hipEvent microseconds per round
    (back-to-back rounds: throughput, not latency; the median of ``--repeats`` windows of ``--launches``).
``pairs``: ``nvrx_comove_pairs`` alone at 4096 ranks, to be run under ``rocprofv3 --kernel-trace --stats`` in a run of its own.
``report``: ``generate_report_from_rings`` + ``identify_stragglers()`` of the headline shape (8 folded ranks x 64 sections x
    10 000 samples) with ``timeline_scores`` on and ``comovement_groups`` off and on, alternating in one process, median and
    p95 of ``--reports`` each; with the option on also the time until ``comovement_groups()`` has returned.
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

from timeline_cost import _alternating  # noqa: E402

ROUND_SHAPES = [(8, 32), (1024, 64), (4096, 64)]  # ranks x buckets
WORK_COLUMNS = 128


def _blocks(rng, R, B):
    """Gathered timeline blocks ``[R, 2, 3, B]``: 8 rows everywhere, levels 1 +- 0.2 %, every other rank 2 % slower on four
    buckets of one of 16 patterns."""
    blocks = np.zeros((R, 2, 3, B), np.float32)
    blocks[:, :, 0] = 8
    blocks[:, :, 1] = 1.0 + 0.002 * rng.standard_normal((R, 2, B))
    for r in range(0, R, 2):
        first = (r // 2 % 16) * (B - 4) // 16
        blocks[r, :, 1, first:first + 4] *= 1.02
    return blocks


def round_(args):
    from nvrx_straggler import _native
    from nvrx_straggler.backend import get_backend

    torch.cuda.set_device(0)
    be = get_backend()
    lib, st = be.lib, be.stream_handle
    rng = np.random.default_rng(0)
    for R, B in ROUND_SHAPES:
        L = _native.table_len(WORK_COLUMNS, 0)
        with torch.cuda.stream(be.stream):
            blocks = torch.from_numpy(_blocks(rng, R, B)).to(be.device)
            out = torch.empty(lib.nvrx_comove_words(R, B), dtype=torch.int32, device=be.device)
            launch = {"comove_groups": lambda: _native.check(lib.nvrx_comove_groups(blocks.data_ptr(), R, B, 8, 10000, 800000,
                                                                                   out.data_ptr(), st))}
            table = torch.from_numpy(rng.lognormal(np.log(100.0), 0.1, (R, L)).astype(np.float32)).to(be.device)
            work = torch.empty(lib.nvrx_work_words(R, WORK_COLUMNS, 0), dtype=torch.int32, device=be.device)
            launch["work_groups"] = lambda: _native.check(lib.nvrx_work_groups(table.data_ptr(), R, WORK_COLUMNS, 0, 0.25, 100000,
                                                                              work.data_ptr(), st))
        be.synchronize()
        res = {"what": "co-movement round", "ranks": R, "B": B, "launches": args.launches, "repeats": args.repeats}
        res.update(_alternating(launch, args, be.stream, be.synchronize))
        rec = out.cpu().numpy().view(np.uint32)[256:256 + 16 * R].reshape(2, R, 8)
        res["groups_of_two_or_more"] = int(((rec[0, :, 0] == np.arange(R)) & (rec[0, :, 1] >= 2)).sum())
        print(json.dumps(res), flush=True)


def pairs(args):
    from nvrx_straggler import _native
    from nvrx_straggler.backend import get_backend

    torch.cuda.set_device(0)
    be = get_backend()
    R = 4096
    x = np.random.default_rng(0).standard_normal((R, 64))
    x = (x / np.sqrt((x * x).sum(axis=1, keepdims=True))).astype(np.float32)
    with torch.cuda.stream(be.stream):
        d_x = torch.from_numpy(x).to(be.device)
        out = torch.empty(be.lib.nvrx_comove_words(R, 64), dtype=torch.int32, device=be.device)
        for _ in range(args.launches):
            _native.check(be.lib.nvrx_comove_pairs(d_x.data_ptr(), R, 800000, out.data_ptr(), be.stream_handle))
    be.synchronize()
    print(json.dumps({"what": "nvrx_comove_pairs", "ranks": R, "launches": args.launches}), flush=True)


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
    gens = {0: ReportGenerator(["relative_perf_scores"], node_name="n", timeline_scores=True),
            1: ReportGenerator(["relative_perf_scores"], node_name="n", timeline_scores=True, comovement_groups=True)}
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
                assert len(rep.comovement_groups()["ranks"]) == local_ranks
            t2 = time.perf_counter_ns()
            if i >= 2 * args.warmup:
                lat[on].append((t1 - t0) * 1e-3)
                if on:
                    readable.append((t2 - t0) * 1e-3)
            be.synchronize()
        out = {"what": "ring report with timelines, call -> flagged set", "reports_each": args.reports, "shape": "8 x 64 x 10000"}
        for on, key in ((0, "off"), (1, "on")):
            out[f"{key}_median_us"] = round(float(np.median(lat[on])), 1)
            out[f"{key}_p95_us"] = round(float(np.percentile(lat[on], 95)), 1)
        out["delta_median_us"] = round(out["on_median_us"] - out["off_median_us"], 1)
        out["comovement_readable_median_us"] = round(float(np.median(readable)), 1)
        print(json.dumps(out), flush=True)
    finally:
        for g in gens.values():
            g.close()
        rings.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["round", "pairs", "report"])
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--reports", type=int, default=50)
    args = ap.parse_args()
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    {"round": round_, "pairs": pairs, "report": report}[args.what](args)


if __name__ == "__main__":
    main()
