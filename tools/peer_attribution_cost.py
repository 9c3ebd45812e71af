#!/usr/bin/env python3
"""What peer attribution costs (docs/MEASUREMENTS.md, "Peer attribution").  One GPU:

    python tools/peer_attribution_cost.py kernels --ranks 8 --ids 64
    python tools/peer_attribution_cost.py kernels --ranks 8 --ids 4096
    python tools/peer_attribution_cost.py kernels --ranks 1024 --ids 128
    python tools/peer_attribution_cost.py report [--reports 200] [--warmup 20]

``kernels``: ``--launches`` rounds of ``nvrx_peer_attribute`` (one launch of ``k_peer_attribute``; the column records it reads
    were written once, ahead of the timing, by ``nvrx_peer_score``) and of the job-wide ``nvrx_attribute``, relative family only
    (its column-minimum launch or launches, then ``k_attribute``), on the SAME table of ``--ranks`` ranks x ``--ids`` kernel ids
    (no sections, every entry present) with ONE group of all ranks and ``min_ranks`` 1, so that both solve the same problem and
    list the same kernels -- checked before anything is timed.  At ``top_n`` 5 and 16, alternating on one stream.  It prints the
    hipEvent time of a round of each (kernels back to back: throughput, not latency), each taken twice so that the spread of
    a step against itself is on the page.
``report``: a synchronous ring report of 8 folded ranks x 64 sections x 10 000 samples with ``peer_groups="block:4"`` and
    ``peer_attribution`` 5 and 0 alternating in one process; median and p95 of ``--reports`` each, call to flagged set (the
    attribution is enqueued and not waited for).
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
    R, K, S = args.ranks, args.ids, 0
    peers = PeerGroups([0] * R)
    rng = np.random.default_rng(0)
    T = np.zeros((R, _native.table_len(K, S)), dtype=np.float32)
    T[:, :K] = rng.lognormal(1.0, 0.5, (R, K))
    T[:, K : 2 * K] = T[:, :K]
    T[:, 2 * K : 3 * K] = rng.uniform(1e3, 1e5, (R, K))
    T[:, -1] = 1.0
    tops = (5, 16)
    with torch.cuda.stream(be.stream):
        table = torch.from_numpy(T).to(be.device)
        block = torch.empty(_native.peer_words(1, R, K, S), dtype=torch.int32, device=be.device)
        scratch = torch.empty(33 * K, dtype=torch.float32, device=be.device)
        out_peer = {n: torch.zeros(_native.peer_attr_words(R, n), dtype=torch.int32, device=be.device) for n in tops}
        out_wide = {n: torch.zeros(_native.attr_words(R, n), dtype=torch.int32, device=be.device) for n in tops}
    d_groups = peers.device(be)
    be.synchronize()
    _native.check(lib.nvrx_peer_score(table.data_ptr(), R, K, S, d_groups.data_ptr(), 1, 0, R, 1, block.data_ptr(), st))

    def per_group(n):
        _native.check(lib.nvrx_peer_attribute(table.data_ptr(), R, K, S, d_groups.data_ptr(), 1, block.data_ptr(), 0, R, 1, n,
                                              out_peer[n].data_ptr(), st))

    def job_wide(n):
        _native.check(lib.nvrx_attribute(table.data_ptr(), R, K, S, 0, R, n, 0, 1, scratch.data_ptr(), out_wide[n].data_ptr(), st))

    steps = [(f"{name}_top{n}", fn, n) for n in tops for name, fn in (("job_wide", job_wide), ("peer", per_group))]
    for _ in range(args.warmup):
        for _, fn, n in steps:
            fn(n)
    be.synchronize()
    for n in tops:  # the same problem: the same kernels, the same scores and lost microseconds
        a = out_peer[n].cpu().numpy().view(np.uint32).reshape(R, 1 + n, 8)[:, 1:, :4]
        b = out_wide[n].cpu().numpy().view(np.uint32).reshape(R, 2, 1 + n, 4)[:, 1, 1:]
        if not (np.array_equal(a[:, :, 0], b[:, :, 0]) and np.array_equal(a[:, :, 2:], b[:, :, 2:])):
            raise SystemExit(f"top_n={n}: the two attributions list different kernels")
    rounds = {name: [] for name, _, _ in steps}
    for name, fn, n in steps * 2:  # alternating, each twice
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(be.stream)
        for _ in range(args.launches):
            fn(n)
        t1.record(be.stream)
        t1.synchronize()
        rounds[name].append(round(t0.elapsed_time(t1) * 1e3 / args.launches, 2))
    print(json.dumps({"what": "kernels", "ranks": R, "kernel_ids": K, "groups": 1, "launches": args.launches,
                      **{name + "_round_us": v for name, v in rounds.items()}}), flush=True)


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
    common = dict(node_name="n", peer_groups="block:4")
    gens = {"off": ReportGenerator(["relative_perf_scores"], **common),
            "on": ReportGenerator(["relative_perf_scores"], peer_attribution=5, **common)}
    lat = {"off": [], "on": []}
    order = ("off", "on", "on", "off")  # each configuration follows itself and the other
    try:
        for i in range(2 * (args.reports + args.warmup)):
            key = order[i % 4]
            rings.set_count_all(samples)
            t0 = time.perf_counter_ns()
            rep = gens[key].generate_report_from_rings(rings, srows, {}, local_ranks=local_ranks)
            rep.identify_stragglers()
            t1 = time.perf_counter_ns()
            if i >= 2 * args.warmup:
                lat[key].append((t1 - t0) * 1e-3)
            be.synchronize()
        out = {"what": "ring report with peer_groups, call -> flagged set", "processes": 1, "reports_each": args.reports,
               "shape": "8 x 64 sections x 10000", "peer_groups": "block:4", "peer_attribution": 5}
        for key in ("off", "on"):
            out[f"{key}_median_us"] = round(float(np.median(lat[key])), 1)
            out[f"{key}_p95_us"] = round(float(np.percentile(lat[key], 95)), 1)
        out["delta_median_us"] = round(out["on_median_us"] - out["off_median_us"], 1)
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
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reports", type=int, default=200)
    args = ap.parse_args()
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    {"kernels": kernels, "report": report}[args.what](args)


if __name__ == "__main__":
    main()
