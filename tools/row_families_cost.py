#!/usr/bin/env python3
"""What the row families cost a report (docs/MEASUREMENTS.md, "Row families").  One GPU:

    python tools/row_families_cost.py [TREE] [--reports 50] [--warmup 5]

``generate_report_from_rings`` + ``identify_stragglers()`` (call -> flagged set) of the headline shape -- 8 folded ranks x 64
sections x 10 000 samples, synchronous -- with all four row families (tail, onset, period, episode scores) off and on,
alternating in one process, as tools/episode_cost.py measures it for one family; median and p95 of ``--reports`` each.
``TREE``: the checkout whose package is measured (default: this one) -- to compare two commits, run this file on both
checkouts in turns.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("tree", nargs="?", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--reports", type=int, default=50)
ap.add_argument("--warmup", type=int, default=5)
args = ap.parse_args()
TREE = os.path.abspath(args.tree)
sys.path[:0] = [os.path.join(TREE, "nvidia-resiliency-ext_amd"), TREE]

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.cuda.set_device(0)
import nvrx_straggler  # noqa: E402
from nvrx_straggler import _native  # noqa: E402
from nvrx_straggler.backend import get_backend  # noqa: E402
from nvrx_straggler.reporting import ReportGenerator  # noqa: E402

assert os.path.abspath(nvrx_straggler.__file__).startswith(TREE + os.sep), nvrx_straggler.__file__
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
ALL = dict(tail_quantile=0.95, onset_detection=True, period_detection=True, episode_detection=True)
gens = {0: ReportGenerator(["relative_perf_scores"], node_name="n"),
        1: ReportGenerator(["relative_perf_scores"], node_name="n", **ALL)}
lat = {0: [], 1: []}
try:
    for i in range(2 * (args.reports + args.warmup)):
        on = i & 1
        rings.set_count_all(samples)
        t0 = time.perf_counter_ns()
        rep = gens[on].generate_report_from_rings(rings, srows, {}, local_ranks=local_ranks)
        rep.identify_stragglers()
        t1 = time.perf_counter_ns()
        if on:
            for fam in ("tail", "onset", "period", "episode"):
                assert len(getattr(rep, fam + "_scores")()["section_relative"]) == sections
        if i >= 2 * args.warmup:
            lat[on].append((t1 - t0) * 1e-3)
        be.synchronize()
    out = {"tree": os.path.relpath(TREE), "reports_each": args.reports}
    for on, key in ((0, "off"), (1, "all_on")):
        out[f"{key}_median_us"] = round(float(np.median(lat[on])), 1)
        out[f"{key}_p95_us"] = round(float(np.percentile(lat[on], 95)), 1)
    print(json.dumps(out), flush=True)
finally:
    for g in gens.values():
        g.close()
    rings.close()
