#!/usr/bin/env python3
"""What ``_nvrx_pyread.flagged`` costs on the host, parent build against this tree's build, side by side in one process
(docs/MEASUREMENTS.md, "Flagged sets reused").  No GPU:

    python tools/flagged_reuse_cost.py --parent-rev HEAD~1            (compiles that revision's csrc/nvrx_pyread.c into a temp dir)
    python tools/flagged_reuse_cost.py --parent-dir DIR               (a directory that holds the parent's _nvrx_pyread*.so)

The headline table: 8 ranks x 64 sections, rank 3 flagged in every column.  Three patterns, ``--calls`` each, ``--rounds`` rounds
with the two builds alternating; microseconds per call, median of the rounds and their spread:
    nothing_flagged   an all-zero table (the call's floor)
    bench_pattern     ``found = flagged(...)``: the previous result dies after the next call has returned, as in bench.py's loop
                      and any training loop; the time includes freeing it
    every_result_held every result appended to a list (cleared outside the timed region): nothing can be reused, every hit copies
Prints one JSON line.
"""
import argparse
import gc
import glob
import importlib.util
import json
import os
import subprocess
import sys
import sysconfig
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "nvidia-resiliency-ext_amd")
SRC = "nvidia-resiliency-ext_amd/csrc/nvrx_pyread.c"
sys.path[:0] = [PKG, REPO]

import numpy as np  # noqa: E402


def _load(directory, tag):
    """The ``_nvrx_pyread`` of ``directory`` under a module name of its own (reporting._load_pyread does the same for
    ``NVRX_DEBUG_LIB_DIR``): both builds live in this process."""
    paths = sorted(glob.glob(os.path.join(directory, "_nvrx_pyread*.so")))
    if not paths:
        raise SystemExit(f"no _nvrx_pyread*.so in {directory}")
    spec = importlib.util.spec_from_file_location(f"{tag}._nvrx_pyread", paths[0])
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _build_rev(rev, out_dir):
    src = subprocess.check_output(["git", "-C", REPO, "show", f"{rev}:{SRC}"])
    c = os.path.join(out_dir, "nvrx_pyread.c")
    with open(c, "wb") as f:
        f.write(src)
    so = os.path.join(out_dir, "_nvrx_pyread" + sysconfig.get_config_var("EXT_SUFFIX"))
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-Wall", "-I" + sysconfig.get_paths()["include"], "-o", so, c])
    return out_dir


class Caller:
    def __init__(self, mod, R=8, S=64, slow=3):
        from nvrx_straggler import reporting

        self.mod, self.R, self.S, self.W = mod, R, S, 2 + 2 * S
        self.ids = [reporting.StragglerId(rank=r, node="n") for r in range(R)]
        self.names = tuple(f"section_{i:03d}" for i in range(S))
        flags = np.zeros((R, self.W), dtype=np.uint8)
        self.zero = flags.tobytes()
        flags[slow, :] = 1
        self.flagged = flags.tobytes()
        self.memo = [None, None, None, None]
        try:
            self(self.flagged)
        except ValueError:  # a build from before the memo kept results
            self.memo = [None, None]
            self(self.flagged)

    def __call__(self, buf):
        return self.mod.flagged(buf, 0, self.R, self.W, self.S, True, True, self.ids, self.names, None, self.memo)


def nothing_flagged(c, calls):
    buf = c.zero
    t0 = time.perf_counter_ns()
    for _ in range(calls):
        found = c(buf)  # noqa: F841
    return (time.perf_counter_ns() - t0) / calls * 1e-3


def bench_pattern(c, calls):
    buf = c.flagged
    found = c(buf)
    found = c(buf)
    t0 = time.perf_counter_ns()
    for _ in range(calls):
        found = c(buf)  # noqa: F841
    return (time.perf_counter_ns() - t0) / calls * 1e-3


def every_result_held(c, calls):
    # the cyclic collector is off while results pile up: its passes over the 130 containers of every held result cost tens of
    # microseconds per call, the same for both builds, and would bury what is compared here
    buf, held, total, batch = c.flagged, [], 0, 500
    gc.disable()
    try:
        for _ in range(0, calls, batch):
            t0 = time.perf_counter_ns()
            for _ in range(batch):
                held.append(c(buf))
            total += time.perf_counter_ns() - t0
            del held[:]
    finally:
        gc.enable()
    return total / (batch * ((calls + batch - 1) // batch)) * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-rev", default="", help="git revision whose csrc/nvrx_pyread.c is the baseline (built into a temp dir)")
    ap.add_argument("--parent-dir", default="", help="directory with the baseline's _nvrx_pyread*.so")
    ap.add_argument("--new-dir", default=os.path.join(PKG, "nvrx_straggler"), help="directory with this tree's _nvrx_pyread*.so")
    ap.add_argument("--calls", type=int, default=20000)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if bool(args.parent_rev) == bool(args.parent_dir):
        ap.error("one of --parent-rev and --parent-dir")
    with tempfile.TemporaryDirectory() as tmp:
        parent_dir = args.parent_dir or _build_rev(args.parent_rev, tmp)
        callers = {"parent": Caller(_load(parent_dir, "parent")), "new": Caller(_load(args.new_dir, "new"))}
        a, b = (c(c.flagged) for c in callers.values())
        assert a == b and list(a[2]) == list(b[2]), "the two builds disagree"
        patterns = (nothing_flagged, bench_pattern, every_result_held)
        gc.collect()
        gc.freeze()  # (as bench.py does before its loop)
        us = {p.__name__: {k: [] for k in callers} for p in patterns}
        for rnd in range(args.rounds + 1):  # (the first round warms both up and is not counted)
            for which in (("parent", "new") if rnd & 1 else ("new", "parent")):
                for p in patterns:
                    v = p(callers[which], args.calls)
                    if rnd:
                        us[p.__name__][which].append(v)
    out = {"what": "_nvrx_pyread.flagged, us per call", "shape": "8 x 64, one rank flagged everywhere", "calls": args.calls,
           "rounds": args.rounds, "memo_len": {k: len(c.memo) for k, c in callers.items()}}
    for name, both in us.items():
        out[name] = {k: {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
                     for k, v in both.items()}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
