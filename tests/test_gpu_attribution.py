"""Kernel attribution on the MI355X: the operator against the NumPy formula, against the score kernel on the same table,
through ReportGenerator on several processes sharing the GPU, and through the Detector's ring path.

Tolerances (from the project, see tests/test_gpu_score.py): share / deficit / explained absolute 2e-6 (f64 sums in another
order, values O(1)); deficit against 1 - score of the score kernel absolute 1e-6 (two f32 roundings of values <= 1);
against the reference's golden scores 1e-4.  Kernel ids are compared exactly, ``score`` and ``lost_us`` bit for bit."""
import numpy as np
import pytest
import torch

import attribution_workers
from attribution_oracle_backend import attribute_table, column_minima
from followup_cases import FOLLOWUP_SHAPES, followup_table
from mp_util import run_ranks
from test_attribution_host import _check_scenario
from test_gpu_score import _random_table
from util import load_golden

pytestmark = pytest.mark.gpu

_TOL = 2e-6
_SHAPES = [(1, 3, 0), (8, 5, 6), (8, 4096, 8), (64, 17, 33), (65, 0, 64), (100, 7, 9), (16, 13000, 40), (4096, 32, 16)]
_PEER_ENV = {"NVRX_EXCHANGE": "peer", "NVRX_REPORT_TIMEOUT_S": "20", "NVRX_DEBUG_PEER_TRIAL_TIMEOUT_S": "5"}


@pytest.fixture(scope="module")
def be():
    from nvrx_straggler.backend import get_backend

    return get_backend()


def _upload(be, T, K, S):
    R = T.shape[0]
    ws = be.workspace(R, K, S, R, 0)
    ws.attr_settle()
    ws.send.copy_(torch.from_numpy(T))
    torch.cuda.synchronize()
    return ws


def _close(g, e, tol, tag, what):
    """NaN masks equal, infinities equal by sign, finite values within ``tol`` (absolute)."""
    assert np.array_equal(np.isnan(g), np.isnan(e)), (tag, what, "NaN")
    inf = np.isinf(e)
    assert np.array_equal(np.isinf(g), inf) and np.array_equal(g[inf], e[inf]), (tag, what, "inf")
    fin = np.isfinite(e)
    err = np.abs(g[fin].astype(np.float64) - e[fin].astype(np.float64))
    assert err.size == 0 or err.max() <= tol, (tag, what, err.max())


def _compare(got, exp, tag, edge_values=False):
    """The kernel's records against the formula's.  ``edge_values``: the table holds zero medians, zero total weights and
    infinities (tests/followup_cases.py), so a LISTED entry may carry a NaN or infinite share, score or lost_us -- compared
    by NaN-ness, by value and sign where infinite, bit for bit where finite; without it a listed entry's share is never NaN
    and score / lost_us are bit-identical throughout."""
    gi, ei = got.view(np.int32), exp.view(np.int32)
    gf, ef = got.view(np.float32), exp.view(np.float32)
    assert got.shape == exp.shape, tag
    assert np.array_equal(gi[:, :, 1:, 0], ei[:, :, 1:, 0]), (tag, "ids", np.argwhere(gi[:, :, 1:, 0] != ei[:, :, 1:, 0])[:8])
    assert np.array_equal(got[:, :, 0, 2], exp[:, :, 0, 2]), (tag, "eligible kernels")
    listed = ei[:, :, 1:, 0] >= 0
    if edge_values:
        nan = np.isnan(ef[:, :, 1:, 2:4])
        assert np.array_equal(np.isnan(gf[:, :, 1:, 2:4]), nan), (tag, "score / lost_us NaN", np.argwhere(np.isnan(gf[:, :, 1:, 2:4]) != nan)[:8])
        assert np.array_equal(got[:, :, 1:, 2:4][~nan], exp[:, :, 1:, 2:4][~nan]), (tag, "score / lost_us bits")  # (inf and the zeros' signs too)
        assert np.isnan(gf[:, :, 1:, 1][~listed]).all() and np.isnan(ef[:, :, 1:, 1][~listed]).all(), tag
        _close(gf[:, :, 1:, 1][listed], ef[:, :, 1:, 1][listed], _TOL, tag, "share")
    else:
        # score and lost_us: the f32 rounding of the f64 formula, bit for bit (NaN where nothing is listed, on both sides)
        assert np.array_equal(got[:, :, 1:, 2:4], exp[:, :, 1:, 2:4]), (tag, "score / lost_us bits")
        assert np.array_equal(np.isnan(gf[:, :, 1:, 1]), ~listed) and np.array_equal(np.isnan(ef[:, :, 1:, 1]), ~listed), tag
        share_err = np.abs(gf[:, :, 1:, 1][listed] - ef[:, :, 1:, 1][listed])
        assert share_err.size == 0 or share_err.max() <= _TOL, (tag, "share", share_err.max())
    for col, what in ((0, "deficit"), (1, "explained")):
        _close(gf[:, :, 0, col], ef[:, :, 0, col], _TOL, tag, what)
    assert np.allclose(gf[:, :, 0, 3], ef[:, :, 0, 3], rtol=1e-6, atol=0), (tag, "W")


@pytest.mark.parametrize("R,K,S", _SHAPES)
def test_operator_matches_the_formula(be, R, K, S):
    rng = np.random.default_rng(R * 1000 + K + S)
    T = _random_table(rng, R, K, S)
    if K >= 4:  # exact ties beyond the ones the data has: two kernels of a rank with equal medians, minima and weights
        T[0, 1], T[0, K + S + 1], T[0, 2 * (K + S) + 1] = T[0, 3], T[0, K + S + 3], T[0, 2 * (K + S) + 3]
    ws = _upload(be, T, K, S)
    full = {}
    for do_indiv, do_rel in ((True, True), (True, False), (False, True)):
        for n in (1, 5, 16):
            got = be.attribute(ws, ws.send, n, do_indiv, do_rel).records()
            exp = attribute_table(T, K, S, n, do_indiv, do_rel)
            _compare(got, exp, (R, K, S, do_indiv, do_rel, n))
            full[(do_indiv, do_rel, n)] = got
            if K == 0:
                assert np.isnan(got.view(np.float32)[:, :, 0, 0]).all() and (got.view(np.int32)[:, :, 1:, 0] == -1).all()
            if not do_rel:
                assert np.isnan(got.view(np.float32)[:, 1, 0, 0]).all() and (got.view(np.int32)[:, 1, 1:, 0] == -1).all()
    # a sub-range of ranks is the slice of the full result
    lo = R // 3
    n_ranks = max(1, min(R - lo, 5))
    part = be.attribute(ws, ws.send, 5, True, True, first_rank=lo, n_ranks=n_ranks).records()
    assert np.array_equal(part.view(np.int32)[:, :, :, 0], full[(True, True, 5)].view(np.int32)[lo : lo + n_ranks, :, :, 0])
    assert np.array_equal(part[:, :, 1:, 2:4], full[(True, True, 5)][lo : lo + n_ranks, :, 1:, 2:4])


def _deficit_check(be, T, table, R, K, S):
    ws = _upload(be, T, K, S)
    be.score(ws, ws.send, True, True)
    scores = ws.scores.copy()
    got = be.attribute(ws, ws.send, 5, True, True).records().view(np.float32)
    for fam in (0, 1):
        deficit, score = got[:, fam, 0, 0].astype(np.float64), scores[:, fam].astype(np.float64)
        assert np.array_equal(np.isnan(deficit), np.isnan(score)), fam
        inf = np.isinf(score)
        assert np.array_equal(np.isinf(deficit), inf) and np.array_equal(deficit[inf], 1.0 - score[inf]), fam
        ok = np.isfinite(score)
        # finite scores to compare wherever the formula has any: always in the individual family and on a "live" table
        alive = fam == 0 or table == "live" or not np.isnan(column_minima(T[:, :K])).all()
        assert ok.any() == alive, (fam, int(ok.sum()))
        if ok.any():
            err = np.abs(deficit[ok] - (1.0 - score[ok])).max()
            print(f"{table} R={R} K={K} S={S} family {fam}: max |deficit - (1 - score)| = {err:.3e} over {int(ok.sum())} ranks")
            assert err <= 1e-6, (fam, err)
        # the listed shares never exceed the deficit, and with every eligible kernel listed they are the deficit
        explained = got[:, fam, 0, 1].astype(np.float64)
        assert (explained[ok] <= deficit[ok] + _TOL).all()


@pytest.mark.parametrize("R,K,S", [(8, 5, 6), (8, 4096, 8), (64, 17, 33), (100, 7, 9), (16, 13000, 40), (4096, 32, 16)])
def test_deficit_is_one_minus_the_score_kernels_score(be, R, K, S):
    """``random``: 15 % of the entries absent independently (from 64 ranks on the relative family has no eligible kernel, and
    the kernel must say so); ``live``: the table of tests/followup_cases.py, whose relative family has finite scores at every
    shape -- with its ordering plants from K = 16 on: some ranks' deficits are NaN or -inf, on both sides."""
    _deficit_check(be, _random_table(np.random.default_rng(R + K + S), R, K, S), "random", R, K, S)
    _deficit_check(be, followup_table("live", R, K, S), "live", R, K, S)


@pytest.mark.parametrize("R,K,S", [s for s in FOLLOWUP_SHAPES if s[1] >= 2])
def test_deficit_is_one_minus_the_score_kernels_score_at_the_boundaries(be, R, K, S):
    _deficit_check(be, followup_table("live", R, K, S), "live", R, K, S)


_SCENARIOS = load_golden("scoring.json")["scenarios"]


@pytest.mark.parametrize("world", [4, 8])
def test_golden_scenarios_with_the_product_backend(world):
    """The scenarios of tests/test_attribution_host.py on processes sharing the GPU, default exchange route (c10d)."""
    batch = [g for g in _SCENARIOS if g["scenario"]["world_size"] == world]
    res = run_ranks(attribution_workers.scoring_scenarios_attributed_batch, world, timeout=300, use_oracle_backend=False,
                    device=0, scenarios=[g["scenario"] for g in batch], cpu=False)
    total = 0
    for i, g in enumerate(batch):
        total += _check_scenario(g, [res[r][i] for r in range(world)])[0]
    assert total > 0


def _check_detector_windows(out):
    first, second = out["windows"]
    assert out["lane_is_none"]
    ex = second["explain"]
    ind = ex["individual"][0]
    assert ind["kernels"], ex
    top = ind["kernels"][0]
    assert top["kernel"].startswith("hipevent::b"), (top, second["kernels"])
    assert top["lost_us"] > 0 and 0 < top["score"] < 0.5 and top["share"] > 0.25
    assert abs(ind["deficit"] - (1.0 - second["indiv"][0])) <= 1e-6, (ind["deficit"], second["indiv"])
    assert ind["num_kernels"] == 2 and len(ind["kernels"]) == 2
    assert abs(ex["relative"][0]["deficit"]) <= 1e-6  # one rank is its own reference
    # the first window: history minimum == this window's median, nothing lost
    assert first["explain"]["individual"][0]["deficit"] == 0.0
    assert [k["kernel"][:11] for k in first["explain"]["individual"][0]["kernels"]] == ["hipevent::a", "hipevent::b"]


@pytest.mark.parametrize("asynchronous", [False, True])
def test_detector_names_the_slowed_section(asynchronous):
    """One process, region timing, kernel_attribution=3, two profile_cuda sections; in the second window section b's GPU work
    is eight times longer.  The wait for the attribution (its one copy-out) happens at ``explain_gpu_scores()``, never in
    ``generate_report`` nor when scores / stragglers are read (counted, not timed)."""
    res = run_ranks(attribution_workers.detector_two_windows, 1, timeout=240, use_oracle_backend=False, device=0,
                    env={"NVRX_GPU_TIMING": "stamp"}, asynchronous=asynchronous, counting=True)
    out = res[0]
    _check_detector_windows(out)
    for w in out["windows"]:
        at_return, before_explain, after_explain = w["copy_outs"]
        assert at_return == before_explain, w["copy_outs"]        # scores and identify_stragglers() read: no wait
        assert after_explain == before_explain + 1, w["copy_outs"]  # the first explain_gpu_scores() is the one wait
    assert out["windows"][0]["copy_outs"][0] == 0


def test_two_processes_over_peer_windows():
    """Ring path over the in-stream peer route (the context entry point, nvrx_report_attribute): rank 1 is ten times slower."""
    res = run_ranks(attribution_workers.detector_peer_two_ranks, 2, timeout=240, use_oracle_backend=False, device=0,
                    env={**_PEER_ENV, "NVRX_GPU_TIMING": "stamp"})
    assert res[0]["route"].startswith("xGMI peer stores") and res[0]["fused"], res[0]["route"]
    assert res[1]["reports"] == [] and len(res[0]["reports"]) == 4
    for t, rep in enumerate(res[0]["reports"]):
        rel = rep["explain"]["relative"]
        assert sorted(rel) == [0, 1]
        assert rel[0]["deficit"] == 0.0 and rel[0]["kernels"][0]["lost_us"] == 0.0, (t, rel[0])
        assert rel[1]["kernels"][0]["kernel"] == "hipevent::work" and rel[1]["kernels"][0]["lost_us"] > 0, (t, rel[1])
        assert rel[1]["deficit"] > 0.3  # ten times the work: nominally 0.9; the two processes share one GPU
        for rr in (0, 1):
            assert abs(rel[rr]["deficit"] - (1.0 - rep["rel"][rr])) <= 1e-6, (t, rr)
            assert abs(rep["explain"]["individual"][rr]["deficit"] - (1.0 - rep["indiv"][rr])) <= 1e-6, (t, rr)


def test_example_names_the_kernels_of_the_slowed_rank():
    """examples/straggler_example.py as a user runs it, NVRX_KERNEL_ATTRIBUTION=5, two ranks sharing the GPU (per-kernel GPU
    timing: real kernel names); from step 60 on rank 1's stand-in kernel takes 1.5x longer.  Rank 0 flags rank 1 and prints the
    kernels that carry its deficit, the stand-in kernel first with most of it."""
    import os
    import re
    import subprocess
    import sys

    from test_gpu_example import REPO, _clean_env

    p = subprocess.run([sys.executable, os.path.join(REPO, "examples", "straggler_example.py"), "--num-processes", "2", "--share-gpu",
                        "--steps", "181", "--report-interval", "60", "--batch-size", "512", "--width", "512", "--slow-rank", "1",
                        "--slow-from", "60", "--slow-by", "simulated", "--threshold", "0.8"],
                       capture_output=True, text=True, timeout=240, env=_clean_env(NVRX_KERNEL_ATTRIBUTION="5"), cwd=REPO)
    assert p.returncode == 0, p.stdout[-2000:] + "\n" + p.stderr[-3000:]
    out = p.stdout
    print(out[-2500:])
    assert re.search(r"step 180: straggler_gpus_relative: \[\(1, ", out), out[-2500:]
    head = re.search(r"step 180:   rank 1: ([\d.]+) of its relative score is missing, ([\d.]+) of it in:", out)
    assert head, out[-2500:]
    deficit, explained = float(head.group(1)), float(head.group(2))
    rel = eval(re.findall(r"step 180: GPUs relative perf: (\{.*\})", out)[-1])
    assert abs(deficit - (1.0 - rel[1])) <= 2e-3  # both printed with three decimals
    block = out[head.end():]
    kernels = re.findall(r"step 180:     (\S.*): share ([\d.]+), score ([\d.]+), (\d+) us above the reference pace", block)
    assert 1 <= len(kernels) <= 10, block[:1500]  # five per family at most
    name, share, score, lost = kernels[0]
    assert float(share) > 0.5 * deficit and float(lost) > 0 and 0.5 < float(score) < 0.8, kernels[0]  # 1 / 1.5
    assert explained <= deficit + 1e-3 and explained >= float(share) - 1e-3
    assert "ncclDev" not in block and "rcclGenericKernel" not in block
    assert "step 60:   rank" not in out  # nobody is flagged in the first window
