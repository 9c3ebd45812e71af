"""GPU parity of the work-group kernels (``k_work_sig``, ``k_work_pairs``, ``k_work_groups``, ``k_work_rank``) and of the
work-group step of a report against the NumPy restatement of tests/work_oracle_backend.py.

Bounds: every word of every part of the block -- signatures, adjacency, partial nearest records, rank records, job record --
bit for bit: each is an integer, or one correctly rounded f64 division converted to f32 (include/nvrx_straggler.h)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import work_workers
from work_cases import CASES
from work_oracle_backend import groups_of, work_block, work_layout

pytestmark = pytest.mark.gpu

PAD, FILL = 64, 0x5A5A5A5A
STAGES = {0: [0, 1, 2, 3], 4: [4, 5, 6, 7]}
SWAPPED = {0: [0, 1, 3, 5], 2: [2, 4, 6, 7]}  # ranks 2 and 5 traded stages


@pytest.fixture(scope="module")
def be():
    from nvrx_straggler.backend import get_backend

    return get_backend()


@functools.lru_cache(maxsize=None)
def _expected(name):
    c = CASES[name]
    return work_block(c["T"], c["K"], c["S"], c["count_tol"], c["max_unlike_ppm"])


def _parts(R, K, S):
    lay = work_layout(R, K, S)
    return {"signatures": (0, lay["adj"]), "adjacency": (lay["adj"], lay["part"]), "partial nearest": (lay["part"], lay["rank"]),
            "rank records": (lay["rank"], lay["job"]), "job record": (lay["job"], lay["words"])}


def _same_block(got, want, R, K, S, tag):
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    for part, (a, b) in _parts(R, K, S).items():
        bad = np.flatnonzero(got[a:b] != want[a:b])
        assert bad.size == 0, (tag, part, bad[:8].tolist(), got[a:b][bad[:8]], want[a:b][bad[:8]])


@pytest.mark.parametrize("name", list(CASES))
def test_the_block_matches_the_restatement_bit_for_bit(be, name):
    from nvrx_straggler import _native

    c = CASES[name]
    T, K, S = c["T"], c["K"], c["S"]
    R = T.shape[0]
    want = _expected(name)
    words = work_layout(R, K, S)["words"]
    assert be.lib.nvrx_work_words(R, K, S) == words == _native.work_words(R, K, S)
    table = torch.from_numpy(T).cuda()
    out = torch.full((PAD + words + PAD,), FILL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = be.lib.nvrx_work_groups(table.data_ptr(), R, K, S, c["count_tol"], c["max_unlike_ppm"], out.data_ptr() + 4 * PAD,
                                 be._stream_handle)
    assert rc == 0, be.lib.nvrx_last_error()
    be.synchronize()
    torch.cuda.synchronize()
    host = out.cpu().numpy().view(np.uint32)
    assert (host[:PAD] == FILL).all() and (host[PAD + words :] == FILL).all(), "a word outside the block was written"
    _same_block(host[PAD : PAD + words], want["words"], R, K, S, name)
    assert np.array_equal(table.cpu().numpy().view(np.uint32), T.view(np.uint32)), "the launch changed the table"
    rank_at = work_layout(R, K, S)["rank"]
    root = host[PAD + rank_at : PAD + rank_at + 8 * R].reshape(R, 8)[:, 0].view(np.int32)
    assert groups_of(root) == c["groups"]  # (the hand-written expectation, not only the restatement's)


def test_the_backend_handle_delivers_rank_records_and_job_record(be):
    c = CASES["chain_of_12"]
    T, K, S = c["T"], c["K"], c["S"]
    R = T.shape[0]
    ws = be.workspace(R, K, S, R, 0)
    ws.work_settle()
    ws.send.copy_(torch.from_numpy(T))
    torch.cuda.synchronize()
    ranks, job = be.work_groups(ws, ws.send, c["count_tol"], c["max_unlike_ppm"]).records()
    want = _expected("chain_of_12")
    assert np.array_equal(ranks, want["ranks"]) and np.array_equal(job, want["job"])
    assert [r for r in range(R) if ranks[r, 2] + 1 < ranks[r, 1]] == c["loose"]


def test_argument_errors_come_back_before_the_device_is_touched(be):
    from nvrx_straggler import _native

    lib = be.lib
    R, K, S = 8, 8, 2
    table = torch.zeros((R, _native.table_len(K, S)), dtype=torch.float32, device="cuda")
    out = torch.full((_native.work_words(R, K, S),), FILL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def groups(tp=table.data_ptr(), R=R, tol=0.25, ppm=100000, op=out.data_ptr()):
        return lib.nvrx_work_groups(tp, R, K, S, tol, ppm, op, be._stream_handle)

    assert groups(tp=None) == _native.ERR_INVALID and groups(op=None) == _native.ERR_INVALID
    assert groups(op=out.data_ptr() + 4) == _native.ERR_INVALID and groups(R=0) == _native.ERR_INVALID
    assert groups(R=_native.WORK_MAX_RANKS + 1) == _native.ERR_RANGE
    assert groups(tol=-0.1) == _native.ERR_RANGE and groups(tol=16.5) == _native.ERR_RANGE and groups(tol=float("nan")) == _native.ERR_RANGE
    assert groups(ppm=-1) == _native.ERR_RANGE and groups(ppm=1000001) == _native.ERR_RANGE
    desc = _native.ReportDesc()
    desc.R, desc.K, desc.S = R, K, S
    assert lib.nvrx_report_work(None, ctypes.byref(desc), 0.25, 100000, out.data_ptr()) == _native.ERR_INVALID
    rings = be.make_rings(1, 4, 16)
    try:  # a context through which no report was issued
        assert lib.nvrx_report_work(rings.ctx, ctypes.byref(desc), 0.25, 100000, out.data_ptr()) == _native.ERR_STATE
    finally:
        rings.close()
    be.synchronize()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == FILL).all()  # nothing was launched


# ---- the work-group step of a report --------------------------------------------------------------------------------------
def test_report_work_behind_a_real_report_equals_the_stateless_entry(be):
    """``nvrx_report_work`` behind the one-call report: the block it leaves is, word for word, what ``nvrx_work_groups`` makes
    of the table that report scored."""
    from nvrx_straggler.folded import FoldedJob

    torch.cuda.set_device(0)
    job = FoldedJob(total_ranks=8, sections=4, ring_cap=64, scores_to_compute=("relative_perf_scores",), node_name="n",
                    kernel_names=work_workers.KERNELS, work_groups=True)
    try:
        for i in range(2):  # the general path, then the one-call report
            for r in range(8):
                sec, kernels = work_workers.stage_window(r)
                job.load(r, sec)
                for name, values in kernels.items():
                    job.rings.push_many(job._no_kernel_rows[name], values, lr=r)
            rep = job.report()
        assert job.reporter._last_plan_fused
        handle = rep.__dict__["_work"].handle
        ws = job.reporter._ring_plan.ws
        R, K, S = ws.R, ws.K, ws.S
        assert (R, K, S) == (8, len(work_workers.KERNELS), 4)
        words = work_layout(R, K, S)["words"]
        ranks, job_rec = handle.records()  # (waits for the step)
        from_report = handle_block = ws.work_buffers()[:words].cpu().numpy().view(np.uint32)
        table = ws.table.clone()
        out = torch.full((words,), FILL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert be.lib.nvrx_work_groups(table.data_ptr(), R, K, S, 0.25, 100000, out.data_ptr(), be._stream_handle) == 0
        be.synchronize()
        stateless = out.cpu().numpy().view(np.uint32)
        _same_block(from_report, stateless, R, K, S, "report against stateless")
        _same_block(handle_block, work_block(table.cpu().numpy(), K, S)["words"], R, K, S, "report against restatement")
        lay = work_layout(R, K, S)
        assert np.array_equal(ranks.reshape(-1), stateless[lay["rank"] : lay["job"]]) and np.array_equal(job_rec, stateless[lay["job"] :])
        assert rep.work_groups()["groups"] == STAGES
    finally:
        job.close()


def _same_scores(a, b):
    """Two peer-score dicts hold the same numbers, NaN where the other has NaN."""
    assert a["gpu_relative"].keys() == b["gpu_relative"].keys()
    for r in a["gpu_relative"]:
        assert np.float32(a["gpu_relative"][r]).view(np.uint32) == np.float32(b["gpu_relative"][r]).view(np.uint32), r
    assert a["section_relative"].keys() == b["section_relative"].keys()
    for n, per_rank in a["section_relative"].items():
        for r, v in per_rank.items():
            assert np.float32(v).view(np.uint32) == np.float32(b["section_relative"][n][r]).view(np.uint32), (n, r)


@pytest.mark.parametrize("asynchronous", [False, True])
def test_auto_peer_groups_equal_explicit_ones_and_name_rank_6_alone(be, asynchronous):
    """The two-stage job folded on one GPU: nobody describes the layout, and ``peer_groups="auto"`` gives the peer scores of
    ``peer_groups="block:4"`` bit for bit -- on the general path and on the one-call report, synchronous and asynchronous."""
    torch.cuda.set_device(0)
    auto = work_workers.folded_two_stages(0, 1, asynchronous=asynchronous, peer_groups="auto")
    told = work_workers.folded_two_stages(0, 1, asynchronous=asynchronous, peer_groups="block:4", work_groups=True)
    assert [r["fused"] for r in auto] == [False, True, True] == [r["fused"] for r in told]
    for i, (a, t) in enumerate(zip(auto, told)):
        assert a["work"]["groups"] == STAGES == t["work"]["groups"], i
        assert a["work"]["singletons"] == [] and not any(v["loose"] for v in a["work"]["ranks"].values())
        assert a["work"]["ranks"][work_workers.SLOW_RANK]["nearest_unlike"] == 0  # slow, not different
        assert a["work"]["ranks"][0] == {"size": 4, "degree": 3, "loose": False, "nearest": 1, "nearest_unlike": 0,
                                         "nearest_columns": 14, "kernels": 10, "sections": 4}
        assert "label_conflicts" not in a["work"] and t["work"]["label_conflicts"] == {}
        assert a["peer"]["groups"] == STAGES and t["peer"]["groups"] == {0: STAGES[0], 1: STAGES[4]}
        _same_scores(a["peer"], t["peer"])
        assert a["job_flagged"] == [4, 5, 6, 7] and a["peer_flagged"] == [work_workers.SLOW_RANK], (i, a["job_flagged"], a["peer_flagged"])
        assert t["peer_flagged"] == [work_workers.SLOW_RANK]


@pytest.mark.parametrize("asynchronous", [False, True])
def test_a_report_held_over_the_next_two_is_still_its_own(be, asynchronous):
    """Report 0 sees two stages of four; from report 1 on ranks 2 and 5 have traded stages.  Read only after all three were
    issued on the same workspace, every report says what ITS table said -- and the labels the user gave contradict the later
    ones."""
    torch.cuda.set_device(0)
    out = work_workers.folded_two_stages(0, 1, asynchronous=asynchronous, swap_at=1, hold=True, work_groups=True,
                                         peer_groups="block:4")
    assert [r["fused"] for r in out] == [False, True, True]
    assert out[0]["work"]["groups"] == STAGES and out[0]["work"]["label_conflicts"] == {}
    for r in out[1:]:
        assert r["work"]["groups"] == SWAPPED
        assert r["work"]["label_conflicts"] == {0: {0: [0, 1, 3], 2: [2]}, 1: {2: [4, 6, 7], 0: [5]}}
    auto = work_workers.folded_two_stages(0, 1, asynchronous=asynchronous, swap_at=1, hold=True, peer_groups="auto")
    assert [r["peer"]["groups"] for r in auto] == [STAGES, SWAPPED, SWAPPED]


def test_the_example_infers_the_two_stages_and_names_rank_6_alone():
    import os
    import re
    import subprocess
    import sys

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(repo, "examples", "straggler_example.py"), "--work"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    job = re.search(r"identify_stragglers\(\): (\[[^\]]*\])", out.stdout)
    peers = re.search(r"identify_peer_stragglers\(\) with peer_groups='auto': (\[[^\]]*\])", out.stdout)
    groups = re.search(r"inferred groups: (\{.*?\}); rule", out.stdout)
    assert job and peers and groups, out.stdout
    assert job.group(1) == "[4, 5, 6, 7]" and peers.group(1) == "[6]", out.stdout
    assert groups.group(1) == "{0: [0, 1, 2, 3], 4: [4, 5, 6, 7]}", out.stdout
    assert "rank 6 (group 4 of 4): 110 kernels, 4 sections; nearest rank 4 differs in 0 of 114 columns" in out.stdout
