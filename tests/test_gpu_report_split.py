"""The synchronous report in two phases on the GPU (nvrx_report_issue -> host work -> nvrx_report_wait):
a folded job of 2 ranks x 4 sections on 64-deep rings reports in the benchmark's pattern (re-arm, report, identify) next to
a second job on the same data that was built with NVRX_DEBUG_REPORT_SPLIT=0, and every report of the two is compared bit for
bit -- scores, flags, statistics rows, flagged sets.  Rows with unequal counts (the scatter launches) and wrapped rings are
part of the pattern."""
import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

R, S, CAP = 2, 4, 64
NAMES = [synth.section_name(s) for s in range(S)]


def _job(monkeypatch, split, **env):
    from nvrx_straggler.folded import FoldedJob

    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if split:
        monkeypatch.delenv("NVRX_DEBUG_REPORT_SPLIT", raising=False)
    else:
        monkeypatch.setenv("NVRX_DEBUG_REPORT_SPLIT", "0")
    job = FoldedJob(total_ranks=R, section_names=NAMES, ring_cap=CAP, node_name="n")
    assert job.reporter._report_split is split
    return job


def _pair(monkeypatch, **env):
    return _job(monkeypatch, True, **env), _job(monkeypatch, False, **env)


def _chunk(t, lr, n):
    """[S, n] samples of step ``t`` for logical rank ``lr``: rank 1 is slow, by a factor that moves with ``t``."""
    return synth.stress_samples(lr + 100 * t, S, n, slow_rank=1 + 100 * t, slow_factor=1.5 + 0.01 * (t % 9))


def _prepare(job, t):
    """The benchmark's re-arm, with what makes the steps differ: fresh samples now and then (appended: rings wrap), rows
    with counts of their own (the statistics kernel then reads the count table behind a scatter)."""
    if t == 0:
        for lr in range(R):
            job.load(lr, _chunk(0, lr, 40))
        return
    job.rearm(48 + 8 * (t % 3))  # 48, 56 or 64 resident samples in every row
    if t % 4 == 1:
        job.rings.set_count(t % S, 17 + t % 20, lr=t % R)
    if t % 7 == 3:
        for lr in range(R):
            job.load(lr, _chunk(t, lr, 16))  # (behind 64 resident samples these wrap the ring)


def _block(job):
    """Private copies of the result block the job's last report wrote: scores, flags, the statistics rows it forwards (those of
    the first logical rank)."""
    ws = job.reporter._ring_plan.ws
    job.backend.wait_seq(ws, ws.seq, stats=True)
    return ws.scores.copy(), ws.flags.copy(), ws.stats[:S].copy()


def _same_block(a, b, what):
    for x, y, name in zip(a, b, ("scores", "flags", "statistics")):
        assert x.tobytes() == y.tobytes(), (what, name, x, y)


def _ranks(found):
    return {k: ({n: {x.rank for x in v2} for n, v2 in v.items()} if isinstance(v, dict) else {x.rank for x in v}) for k, v in found.items()}


def _read(rep):
    exact = lambda m: {k: float(v).hex() for k, v in m.items()}  # noqa: E731
    return ({n: exact(rep.section_relative_perf_scores[n]) for n in NAMES},
            {n: exact(rep.section_individual_perf_scores[n]) for n in NAMES},
            {n: exact(rep.local_section_summaries[n]) for n in NAMES}, _ranks(rep.identify_stragglers()))


def _steps(monkeypatch, n_steps, **env):
    a, b = _pair(monkeypatch, **env)
    try:
        flagged_any = False
        for t in range(n_steps):
            _prepare(a, t)
            rep_a = a.report()
            found_a = rep_a.identify_stragglers()
            if t:  # (step 0 learns the names on the general path and builds the plan)
                blk_a = _block(a)
            _prepare(b, t)
            rep_b = b.report()
            found_b = rep_b.identify_stragglers()
            assert _ranks(found_a) == _ranks(found_b), t
            if t:
                _same_block(blk_a, _block(b), t)
                assert not np.isnan(blk_a[0][:, 2:]).any(), t
            flagged_any = flagged_any or bool(found_a["straggler_sections_relative"])
            for job in (a, b):
                assert all(job.rings.count(row, lr) == 0 for lr in range(R) for row in range(S)), t  # report(reset=True)
        assert flagged_any
        return a, b
    except BaseException:
        a.close(), b.close()
        raise


def test_fifty_reports_equal_the_one_call_paths_bit_for_bit(monkeypatch):
    a, b = _steps(monkeypatch, 50)
    a.close(), b.close()


def test_without_the_resident_scorer(monkeypatch):
    """NVRX_DEBUG_RESIDENT_SCORER=0 (read when the context is created): the score kernel is queued behind the statistics
    kernel, and nvrx_report_wait takes its other tail."""
    a, b = _steps(monkeypatch, 6, NVRX_DEBUG_RESIDENT_SCORER="0")
    a.close(), b.close()


def test_a_held_report_and_late_samples(monkeypatch):
    """A Report held across the next two reports still reads its own values; samples pushed from another stream right after
    ``report()`` returned are not in that report."""
    import torch

    a, b = _pair(monkeypatch)
    try:
        held, want = [], []
        for t in range(5):
            _prepare(a, t)
            held.append(a.report())  # nothing of it is read yet
            _prepare(b, t)
            want.append(_read(b.report()))
        for t in range(5):  # (every block has been written again since, reports 0..2 twice)
            assert _read(held[t]) == want[t], t
        assert want[1] != want[2]

        # late samples: the rings are full (64 of 64), so whatever is pushed now overwrites the window's oldest samples
        for job in (a, b):
            job.rearm(CAP)
        rep = a.report(reset=False)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            late = torch.full((S, 32), 1.0e6, dtype=torch.float32, device=a.backend.device)
        side.synchronize()
        for lr in range(R):
            rc = a.rings.lib.nvrx_ring_push_device_rows(a.rings.ctx, lr * S, S, late.data_ptr(), 32, late.stride(0), side.cuda_stream)
            assert rc == 0
        side.synchronize()
        assert _read(rep) == _read(b.report(reset=False))
        a.backend.synchronize()
    finally:
        a.close(), b.close()


def test_wait_and_issue_out_of_turn(monkeypatch):
    """The state errors of the two entry points that need a context: a wait with nothing pending, a second issue, a wait
    with another descriptor (which gives the pending report up); and the job reports as before afterwards."""
    from nvrx_straggler import _native

    a, b = _pair(monkeypatch)
    try:
        for t in range(2):
            for job in (a, b):
                _prepare(job, t)
                job.report()
        lib, ctx, be = a.rings.lib, a.rings.ctx, a.backend
        gen = a.reporter
        ws = gen._ring_plan.ws
        assert lib.nvrx_report_wait(ctx, ws.block.desc_ref) == _native.ERR_STATE
        assert b"no report is pending" in lib.nvrx_last_error()
        a.rearm(40)
        ws.settle_readers()
        seq = a.rings.report_issue(ws, S, S, True, True, gen.thresholds)
        blk, other = ws.block, ws.blocks[1 - ws._cur]
        assert lib.nvrx_report_issue(ctx, other.desc_ref, be._stream_handle) == _native.ERR_STATE
        assert b"pending" in lib.nvrx_last_error()
        assert lib.nvrx_report_wait(ctx, other.desc_ref) == _native.ERR_STATE
        assert b"another descriptor" in lib.nvrx_last_error()
        assert lib.nvrx_report_wait(ctx, blk.desc_ref) == _native.ERR_STATE  # nothing is pending after any return
        # the abandoned report still runs: see it land before the block is anybody's again
        be.wait_seq(ws, seq, block=blk)
        be.wait_seq(ws, seq, stats=True, block=blk)
        ws.mark_live(seq)
        issued = (ws.scores.copy(), ws.flags.copy(), ws.stats[:S].copy())
        b.rearm(40)
        b.report(reset=False)
        _same_block(issued, _block(b), "issued by hand")
        a.rings.reset(), b.rings.reset()
        for t in range(2, 5):
            _prepare(a, t)
            _prepare(b, t)
            assert _read(a.report()) == _read(b.report()), t
    finally:
        a.close(), b.close()


def test_every_option_on_the_split_report_equals_the_one_call(monkeypatch):
    """The job of tests/full_report_script.py -- 8 folded ranks, 3 sections, rings 256 deep, every option on, synchronous --
    for three windows, once on the two-call route and once with NVRX_DEBUG_REPORT_SPLIT=0, each in a generator and a
    workspace of its own (the backend caches workspaces per shape: the two jobs differ in their rows per rank).  The same
    kernels run on the same table behind either route's report, in the same order, so every reader says the same bit for bit
    (``same``: NaN equal to NaN) and the same ranks are identified."""
    import full_report_script as fs
    from nvrx_straggler.backend import get_backend

    be, said = get_backend(), {}
    for split, rows_per_rank in ((True, fs.ROWS_PER_RANK + 2), (False, fs.ROWS_PER_RANK + 3)):
        monkeypatch.setenv("NVRX_DEBUG_REPORT_SPLIT", "1" if split else "0")
        job = fs.Job(be, rows_per_rank=rows_per_rank)
        try:
            assert job.gen._report_split is split
            issued, issue = [], job.rings.report_issue
            monkeypatch.setattr(job.rings, "report_issue", lambda *a, **kw: issued.append(1) or issue(*a, **kw))
            said[split] = []
            for w in range(3):
                rep = job.report(w)
                said[split].append((fs.read(rep), fs.identified(rep)))
            assert len(issued) == (2 if split else 0)  # (window 0 learns the names on the general path)
        finally:
            job.close()
    for w in range(3):
        assert fs.same(said[True][w][0], said[False][w][0]), (w, said[True][w][0], said[False][w][0])
        assert said[True][w][1] == said[False][w][1], w
    assert all(said[True][2][1][m] for m in ("identify_slack_stragglers", "identify_pace_stragglers", "identify_onset_stragglers"))
    assert not fs.same(said[True][1][0], said[True][2][0])  # (the windows differ: equal results are not one result twice)
