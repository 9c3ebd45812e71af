"""GPU parity of the tail kernels (``k_row_quantile``, ``k_tail_score``) and of the tail step of a report against the NumPy
restatement of tests/tail_oracle_backend.py.  Every row of every case is compared."""
import numpy as np
import pytest
import torch

from tail_oracle_backend import row_quantile, tail_scores_table
from test_gpu_score import _random_table

pytestmark = pytest.mark.gpu

COUNTS = (0, 1, 2, 3, 7, 63, 64, 65, 255, 4095, 4096, 4097, 8192, 10000, 65535, 65536)
Q_PPMS = (500000, 900000, 950000, 990000, 999999)
ROWS = 64


@pytest.fixture(scope="module")
def be():
    from nvrx_straggler.backend import get_backend

    return get_backend()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _quantile(be, samples, counts, q_ppm):
    s = torch.from_numpy(np.ascontiguousarray(samples, dtype=np.float32)).cuda()
    c = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int32)).cuda()
    return be.row_quantile(s, c, q_ppm).cpu().numpy()


def _med(be, samples, counts):
    s = torch.from_numpy(np.ascontiguousarray(samples, dtype=np.float32)).cuda()
    c = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int32)).cuda()
    return be.row_stats(s, c, None).cpu().numpy()[:, 2]


def _data(kind, rng, rows, stride):
    """[rows, stride] f32 of one data kind (the whole stride is filled: a row's count picks its prefix)."""
    timings = rng.lognormal(np.log(1000.0), 0.02, (rows, stride)).astype(np.float32)
    if kind == "lognormal":
        return timings
    if kind == "equal":
        return np.repeat(rng.lognormal(1.0, 1.0, (rows, 1)).astype(np.float32), stride, axis=1)
    if kind == "two_values":
        lo = rng.lognormal(1.0, 0.5, (rows, 1)).astype(np.float32)
        return np.where(rng.random((rows, stride)) < 0.93, lo, lo * np.float32(1.5)).astype(np.float32)
    if kind == "ascending":
        return (np.float32(10.0) + np.arange(stride, dtype=np.float32)[None, :] * rng.uniform(0.001, 1.0, (rows, 1)).astype(np.float32))
    if kind == "descending":
        return np.ascontiguousarray(_data("ascending", rng, rows, stride)[:, ::-1])
    if kind == "outliers":
        return np.where(rng.random((rows, stride)) < 0.01, timings * np.float32(1000.0), timings).astype(np.float32)
    if kind == "wide":
        return (10.0 ** rng.uniform(-30.0, 30.0, (rows, stride))).astype(np.float32)
    if kind == "denormals":
        u = rng.integers(0, 0x00800000, (rows, stride), dtype=np.uint32)  # (zeros and the smallest normal's neighbours included)
        return u.view(np.float32)
    if kind == "some_inf":
        return np.where(rng.random((rows, stride)) < 0.1, np.float32(np.inf), timings).astype(np.float32)
    if kind == "only_inf":
        m = timings.copy()
        m[::2] = np.inf  # every other row is +inf throughout
        return m
    if kind == "signed":
        m = rng.normal(0.0, 1.0, (rows, stride)).astype(np.float32)
        pick = rng.random((rows, stride))
        m[pick < 0.05] = -np.inf
        m[(pick >= 0.05) & (pick < 0.25)] = -0.0
        m[(pick >= 0.25) & (pick < 0.45)] = 0.0
        return m
    if kind == "nan":
        m = timings.copy()
        m[rng.random((rows, stride)) < 0.05] = np.float32(np.nan)  # 0x7FC00000: the sign bit is clear
        assert not (_bits(m[np.isnan(m)]) >> 31).any()
        return m
    raise AssertionError(kind)


DATA_KINDS = ("lognormal", "equal", "two_values", "ascending", "descending", "outliers", "wide", "denormals", "some_inf",
              "only_inf", "signed", "nan")


def _check(be, m, counts, q_ppm, tag):
    got = _quantile(be, m, counts, q_ppm)
    exp = row_quantile(m, counts, q_ppm)
    bad = np.flatnonzero(_bits(got) != _bits(exp))
    assert bad.size == 0, (tag, q_ppm, bad[:8].tolist(), [int(counts[i]) for i in bad[:8]], got[bad[:8]], exp[bad[:8]])
    if q_ppm == 500000:
        clean = np.array([c > 0 and not np.isnan(m[r, : int(c)]).any() for r, c in enumerate(counts)])
        if clean.any():
            med = _med(be, m, counts)
            bad = np.flatnonzero(clean & (_bits(med) != _bits(got)))
            assert bad.size == 0, (tag, "MED", bad[:8].tolist(), med[bad[:8]], got[bad[:8]])


@pytest.mark.parametrize("kind", DATA_KINDS)
@pytest.mark.parametrize("stride", [4096, 65536])
def test_row_quantile_bit_exact(be, kind, stride):
    """counts x q x data: 64 rows per launch, every row with its own count (the 16 counts four times over; those a stride
    cannot hold are clipped to it, as the kernel clips them)."""
    rng = np.random.default_rng(sum(map(ord, kind)) + stride)
    m = _data(kind, rng, ROWS, stride)
    counts = np.minimum(np.array(COUNTS * 4, dtype=np.int64), stride).astype(np.uint32)
    rng.shuffle(counts)
    for q_ppm in Q_PPMS:
        _check(be, m, counts, q_ppm, (kind, stride))


@pytest.mark.parametrize("stride", [4, 8, 64, 256, 1000, 1024, 2048, 3072, 4096, 5000, 8192, 10000, 16384, 20480, 32768, 65536])
def test_row_quantile_every_row_stride(be, stride):
    rng = np.random.default_rng(stride)
    m = _data("lognormal", rng, ROWS, stride)
    m[1::4] = _data("two_values", rng, ROWS, stride)[1::4]
    m[2::4] = _data("signed", rng, ROWS, stride)[2::4]
    counts = np.full(ROWS, min(1000, stride), dtype=np.uint32)
    counts[3::8] = rng.integers(0, min(1000, stride) + 1, counts[3::8].size)
    for q_ppm in Q_PPMS:
        _check(be, m, counts, q_ppm, ("stride", stride))


@pytest.mark.parametrize("rows,stride", [(1, 10000), (512, 10000), (4096, 1000)])
def test_row_quantile_launch_sizes(be, rows, stride):
    rng = np.random.default_rng(rows)
    m = _data("lognormal", rng, rows, stride)
    m[::7] = _data("outliers", rng, rows, stride)[::7]
    counts = np.full(rows, stride, dtype=np.uint32)
    counts[5::11] = rng.integers(0, stride + 1, counts[5::11].size)
    for q_ppm in (500000, 950000, 999999):
        _check(be, m, counts, q_ppm, ("launch", rows, stride))


def _random_tails(rng, R, K, S, p_missing=0.15):
    t = rng.lognormal(1.0, 0.5, (R, K + S)).astype(np.float32)
    t[rng.random((R, K + S)) < p_missing] = -1.0
    return t


def _tail_score(be, tails, T, K, S, first_rank=0, n_ranks=None):
    R = T.shape[0]
    ws = be.workspace(R, K, S, R, 0)
    ws.tail_settle()
    ws.send.copy_(torch.from_numpy(T))
    _, table, _, _ = ws.tail_buffers()
    if table.numel():
        table.copy_(torch.from_numpy(tails))
    torch.cuda.synchronize()
    handle = be.tail_score(ws, table, ws.send, first_rank, n_ranks, 950000)
    got_tails, scores = handle.records()
    lo = first_rank
    hi = R if n_ranks is None else first_rank + n_ranks
    assert np.array_equal(_bits(got_tails), _bits(tails[lo:hi]))
    return scores


@pytest.mark.parametrize("R,K,S", [(1, 3, 0), (8, 5, 6), (8, 4096, 8), (64, 17, 33), (65, 0, 64), (100, 7, 9), (4096, 32, 16)])
def test_tail_score_matches_numpy(be, R, K, S):
    rng = np.random.default_rng(R * 1000 + K + S)
    T = _random_table(rng, R, K, S)
    tails = _random_tails(rng, R, K, S)
    if R > 1 and K + S > 2:
        tails[0, 0] = 0.0  # a zero tail: inf / NaN, never an exception
        tails[:, 1] = rng.lognormal(1.0, 0.5, R)  # a column nobody misses
    got = _tail_score(be, tails, T, K, S)
    exp = tail_scores_table(tails, T, K, S)
    assert got.shape == exp.shape == (R, 1 + S)
    assert np.array_equal(np.isnan(got), np.isnan(exp))
    sec_ok = ~np.isnan(exp[:, 1:])
    assert np.array_equal(_bits(got[:, 1:][sec_ok]), _bits(exp[:, 1:][sec_ok]))  # one f64 quotient rounded to f32
    gpu_ok = np.isfinite(exp[:, 0])
    assert np.array_equal(np.isinf(got[:, 0]), np.isinf(exp[:, 0]))
    if gpu_ok.any():
        assert np.abs(got[gpu_ok, 0].astype(np.float64) - exp[gpu_ok, 0].astype(np.float64)).max() <= 2e-6
    # a sub-range of ranks equals the slice of the full result
    lo, n = (R // 3, max(1, R // 2)) if R > 1 else (0, 1)
    part = _tail_score(be, tails, T, K, S, lo, n)
    assert np.array_equal(_bits(part), _bits(got[lo : lo + n]))


# ---- the tail step of a report --------------------------------------------------------------------------------------------
import math  # noqa: E402

import tail_workers  # noqa: E402
from mp_util import run_ranks  # noqa: E402
from tail_oracle_backend import tail_rank  # noqa: E402

_NAMES = [f"section_{s:03d}" for s in range(64)]


def _check_headline(rep, data, explained=()):
    assert rep["median_flagged"] == [], rep["median_flagged"]
    assert rep["tail_gpus"] == []
    assert sorted(rep["tail_sections"]) == _NAMES and all(v == [3] for v in rep["tail_sections"].values())
    assert rep["explained"] == list(explained)
    t = rep["tails"]
    assert t["quantile"] == 0.95 and t["kernel_tails"] == {}
    k = tail_rank(950000, 10000)
    exp = np.sort(data, axis=2)[:, :, k]  # [8, 64]: positive samples, NumPy's order is the keys' order
    ref = exp.min(axis=0)
    for s, n in enumerate(_NAMES):
        for r in range(8):
            assert t["section_tails"][n][r] == float(exp[r, s]), (n, r)
            want = float(np.float32(np.float64(ref[s]) / np.float64(exp[r, s])))
            assert t["section_relative"][n][r] == want, (n, r)
            assert (0.68 <= want <= 0.70) if r == 3 else want >= 0.99, (n, r, want)


def test_headline_shape_in_one_process(be):
    data = tail_workers.headline_data()
    out = tail_workers.folded_headline(0, 1)
    assert len(out) == 3
    for rep in out:
        _check_headline(rep, data)


@pytest.mark.parametrize("world,attribution", [(4, 3), (8, 0)])
def test_headline_shape_on_processes_sharing_the_gpu(world, attribution):
    """Default route (gloo / c10d); with four processes kernel attribution is on as well: both follow-up launches behind one
    report, both read later."""
    data = tail_workers.headline_data()
    res = run_ranks(tail_workers.folded_headline, world, timeout=420, use_oracle_backend=False, device=0,
                    kernel_attribution=attribution)
    assert all(r == [None] * 3 for r in res[1:])
    for rep in res[0]:
        _check_headline(rep, data, explained=("relative",) if attribution else ())


@pytest.mark.parametrize("asynchronous", [False, True])
def test_next_window_written_from_another_stream_right_after_the_report(asynchronous):
    """The ordering rule: the quantile kernel has read its window before the report call returns."""
    res = run_ranks(tail_workers.ring_windows_written_from_another_stream, 1, timeout=300, use_oracle_backend=False, device=0,
                    asynchronous=asynchronous)[0]
    samples, names = res["samples"], res["names"]
    assert len(res["reports"]) == samples.shape[0] == 40
    k = tail_rank(900000, samples.shape[2])
    for w, rep in enumerate(res["reports"]):
        exp = np.sort(samples[w], axis=1)[:, k]
        got = np.array([rep["section_tails"][n] for n in names], dtype=np.float32)
        assert np.array_equal(_bits(got), _bits(exp)), (w, got, exp)
        assert all(v == 1.0 for v in rep["section_relative"].values())
        at_return, before, after_first, after_second = rep["copy_outs"]
        # neither the report call nor scores / stragglers copy tails out; the first tail_scores() does, exactly once
        # (an unread predecessor costs its own copy when its buffers are reused: every report here is read)
        assert at_return == before == w and after_first == after_second == w + 1, (w, rep["copy_outs"])


def test_detector_shows_a_bursty_section_in_its_tail():
    res = run_ranks(tail_workers.detector_bursty_section, 1, timeout=300, use_oracle_backend=False, device=0,
                    env={"NVRX_GPU_TIMING": "stamp"})[0]
    assert res["lane_is_none"]
    for w in res["windows"]:
        t = w["tails"]
        assert t["quantile"] == 0.9 and t["gpu_relative"] == {0: 1.0} and w["tail_stragglers"]
        assert all(v == {0: 1.0} for v in t["section_relative"].values())
        key = next(k for k in t["kernel_tails"] if k.startswith("hipevent::bursty"))
        steady = next(k for k in t["kernel_tails"] if k.startswith("hipevent::steady"))
        print("bursty: tail", t["kernel_tails"][key][0], "median", w["med"][key], "| steady: tail",
              t["kernel_tails"][steady][0], "median", w["med"][steady])
        assert t["kernel_tails"][key][0] > 2.0 * w["med"][key], (t["kernel_tails"][key], w["med"][key])


def test_two_processes_asking_for_peer_windows_stay_on_c10d():
    from test_gpu_attribution import _PEER_ENV

    res = run_ranks(tail_workers.detector_peer_with_tails, 2, timeout=300, use_oracle_backend=False, device=0,
                    env={**_PEER_ENV, "NVRX_GPU_TIMING": "stamp"})
    for r in res:
        assert r["mode"] == "c10d" and not r["direct"], r["route"]
        assert len(r["ignored_lines"]) == 1, r["ignored_lines"]
    assert res[1]["reports"] == [] and len(res[0]["reports"]) == 3
    for rep in res[0]["reports"]:
        t = rep["tails"]
        assert sorted(t["gpu_relative"]) == [0, 1]
        work = t["kernel_tails"]["hipevent::work"]
        # rank 1 does ten times the work on every third entry: its 0.9 quantile is a slow entry, its median is not
        assert work[1] > 3.0 * work[0], work
        want = min(work.values()) / work[1]
        assert abs(t["gpu_relative"][1] - want) <= 2e-6 and abs(t["gpu_relative"][0] - min(work.values()) / work[0]) <= 2e-6
        assert t["gpu_relative"][1] < 0.5 < rep["rel"][1], (t["gpu_relative"], rep["rel"])


def test_example_prints_the_intermittently_slow_rank_as_a_tail_straggler():
    """examples/straggler_example.py as tests/test_gpu_attribution.py runs it, with --slow-by intermittent (every 5th step of
    rank 1 from step 60 on) and NVRX_TAIL_QUANTILE=0.9: at step 180 rank 1 is a tail GPU straggler and no median-based one."""
    import os
    import re
    import subprocess
    import sys

    from test_gpu_example import REPO, _clean_env

    p = subprocess.run([sys.executable, os.path.join(REPO, "examples", "straggler_example.py"), "--num-processes", "2", "--share-gpu",
                        "--steps", "181", "--report-interval", "60", "--batch-size", "512", "--width", "512", "--slow-rank", "1",
                        "--slow-from", "60", "--slow-by", "intermittent", "--threshold", "0.8"],
                       capture_output=True, text=True, timeout=240, env=_clean_env(NVRX_TAIL_QUANTILE="0.9"), cwd=REPO)
    assert p.returncode == 0, p.stdout[-2000:] + "\n" + p.stderr[-3000:]
    out = p.stdout
    print(out[-2500:])
    rel = eval(re.findall(r"step 180: GPUs relative perf: (\{.*\})", out)[-1])
    tail = eval(re.findall(r"step 180: GPUs relative tail perf \(q=0.9\): (\{.*\})", out)[-1])
    print("step 180: median-based", rel, "tail", tail)
    assert re.search(r"step 180: tail straggler_gpus_relative: \[\(1, ", out), out[-2500:]
    assert "step 180: straggler_gpus_relative" not in out
    assert tail[1] < tail[0] and tail[1] <= rel[1] - 0.1
