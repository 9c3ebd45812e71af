"""bench.py --dump-outputs: what the timed step returned, written as .npy -- the four score mappings, the local statistics and
the flagged sets of a real Report.  CPU-only: the report comes from the checker backend (tests/oracle_backend.py) in a child
interpreter of its own, on the benchmark's seeded inputs cut down to 4 sections x 200 samples."""
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = r"""
import json, os, sys
for p in (REPO, os.path.join(REPO, "nvidia-resiliency-ext_amd"), os.path.join(REPO, "tests"), os.path.join(REPO, "tests", "golden")):
    sys.path.insert(0, p)
import bench, synth
from nvrx_straggler import backend
from oracle_backend import OracleBackend
backend.set_backend(OracleBackend())
from nvrx_straggler.folded import FoldedJob

out_dir = sys.argv[1]
names = [synth.section_name(s) for s in range(4)]
job = FoldedJob(total_ranks=8, section_names=names, ring_cap=200, node_name="node0")
written = []
for k in range(2):  # two reports over the same inputs
    for lr, r in enumerate(job.logical_ranks()):
        x = synth.stress_samples(r, 4, 200, slow_rank=3, slow_factor=1.5)
        for s, name in enumerate(names):
            job.rings.push_many(job.rows[name], x[s], lr=lr)
    rep = job.report()
    written.append(bench._dump_outputs(os.path.join(out_dir, str(k)), rep, rep.identify_stragglers(), names))
print("WRITTEN " + json.dumps(written), flush=True)
"""

# (no gpu_*_perf_scores: the job times no GPU work, those mappings are NaN for every rank and are not written)
FILES = ["local_section_summaries", "section_individual_perf_scores", "section_relative_perf_scores", "straggler_gpus_individual",
         "straggler_gpus_relative", "straggler_sections_individual", "straggler_sections_relative"]


def test_dump_outputs_writes_the_reports_arrays_and_they_repeat_on_the_same_inputs(tmp_path):
    r = subprocess.run([sys.executable, "-c", f"REPO = {REPO!r}\n" + SCRIPT, str(tmp_path)], capture_output=True, text=True,
                       timeout=300, cwd=REPO)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("WRITTEN ")]
    assert r.returncode == 0 and len(lines) == 1, (r.stdout[-1500:], r.stderr[-1500:])
    assert json.loads(lines[0][len("WRITTEN "):]) == [FILES, FILES]
    assert sorted(os.listdir(tmp_path / "0")) == sorted(f + ".npy" for f in FILES)
    a = {f: np.load(tmp_path / "0" / (f + ".npy")) for f in FILES}
    b = {f: np.load(tmp_path / "1" / (f + ".npy")) for f in FILES}
    for f in FILES:
        assert a[f].dtype in (np.float32, np.float64) and np.isfinite(a[f]).all(), f
        assert a[f].shape == b[f].shape and np.array_equal(a[f], b[f]), f
    # scores: [sections, ranks]; logical rank 3 runs x1.5 slower in every section
    rel = a["section_relative_perf_scores"]
    assert rel.shape == a["section_individual_perf_scores"].shape == (4, 8)
    assert np.all(np.abs(rel[:, 3] - 1 / 1.5) < 0.02) and np.all(np.delete(rel, 3, axis=1) > 0.97)
    assert np.all(a["section_individual_perf_scores"] == 1.0)
    # flagged sets at the default thresholds as 0/1 tables
    expect = np.zeros((4, 8), dtype=np.float32)
    expect[:, 3] = 1
    assert np.array_equal(a["straggler_sections_relative"], expect)
    assert not a["straggler_sections_individual"].any() and not a["straggler_gpus_relative"].any()
    assert a["straggler_gpus_relative"].shape == a["straggler_gpus_individual"].shape == (8,)
    # this process's statistics (logical rank 0): MIN, MAX, MED, AVG, STD, NUM in Statistic order, against the C oracle
    from oracle import oracle
    import synth

    st = a["local_section_summaries"]
    x = synth.stress_samples(0, 4, 200, slow_rank=3, slow_factor=1.5)
    assert st.shape == (4, 6)
    for s in range(4):
        exp = oracle.section_stats(x[s].astype(np.float64))
        assert st[s, 0] == np.float32(exp[0]) and st[s, 1] == np.float32(exp[1]) and st[s, 2] == np.float32(exp[2])
        assert abs(st[s, 3] - exp[3]) <= 1e-6 * abs(exp[3]) and st[s, 5] == 200
