"""GPU parity of the slack scores per peer group (``k_slack_group_cols``, ``k_slack_rank<true>``, ``k_slack_group_job`` in its
three forms) through the C ABI and the backend, and of the slack step of a report with ``slack_peer_groups``, against the
restatement of tests/slack_group_oracle_backend.py.  Every record of every case is compared.

Bounds: pair records, counts and group ids bit for bit (a minimum, its holder and counts); the floats of rank and group records
within 2e-6 * max(1, |expected|) with equal NaN and inf masks, tests/test_gpu_slack.py's bound for f64 sums taken in another
order; inputs with power-of-two counts and integer per-call times have exact quotients and sums and are compared bit for bit.

``max_group`` has to lie in 1..R, so a second run with ``max_group = 65`` exists only for tables of 65 ranks and more: the shapes
whose groups all fit a wave and whose table is larger run once with their true ``max_group`` (the one-wave group kernel) and
once with a larger one (the 256- or 1024-thread select), and the two blocks are equal word for word."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from score_cases import random_table
from slack_group_oracle_backend import ALLREDUCE, RANKS, SENDRECV, TWO_SIX, groups_array, play_stages, slack_group_records
from slack_oracle_backend import COLS, NAN_BITS, column_of, named, slack_records
from test_gpu_slack import _exact_table, _slack_table

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD, FILL = 64, 0x5A5A5A5A


@pytest.fixture(scope="module")
def be():
    from nvrx_straggler.backend import get_backend

    return get_backend()


def _labels(kind, R):
    if kind == "one":
        return [0] * R
    if kind == "2+6":
        return list(TWO_SIX)
    if kind == "singletons":
        return list(range(R))
    if kind == "65+1":  # the singleton in the middle: members[] is no identity
        return [1 if r == 7 else 0 for r in range(R)]
    if kind == "64+65+1":
        return [2 if r == 101 else (0 if r % 2 == 0 and r < 128 else 1) for r in range(R)]
    if kind == "1025+1":
        return [1 if r == 513 else 0 for r in range(R)]
    if kind.startswith("mod:"):
        return [r % int(kind[4:]) for r in range(R)]
    raise KeyError(kind)


# (R, groups): the smallest either side of each switch of k_slack_group_job, and small groups riding the larger variants
SHAPES = [(1, "one"), (8, "2+6"), (8, "mod:2"), (8, "singletons"), (64, "one"), (66, "65+1"), (130, "64+65+1"), (1026, "1025+1")]
# shapes whose groups fit a wave in a table large enough for a larger max_group: (R, groups, the larger max_group)
BOTH = [(66, "mod:2", 65), (130, "mod:4", 65), (1026, "mod:32", 1025)]


def _run(be, slack, T, K, S, gh, G, max_group, min_ranks, min_peers):
    """The entry on a guard-padded buffer: ``(groups, pairs, ranks)`` of all R ranks."""
    from nvrx_straggler import _native

    R = slack.shape[0]
    words = _native.slack_group_words(G, R)
    assert words == 8 * G + 256 * G + 8 * R
    d_slack = torch.from_numpy(np.ascontiguousarray(slack.reshape(R, 2 * COLS))).cuda()
    d_table = torch.from_numpy(T).cuda() if K > 0 else None
    d_groups = torch.from_numpy(np.asarray(gh, dtype=np.int32)).cuda()
    out = torch.full((PAD + words + PAD,), FILL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = be.lib.nvrx_slack_group_score(d_slack.data_ptr(), d_table.data_ptr() if K > 0 else None, R, K, S, d_groups.data_ptr(), G,
                                       max_group, min_ranks, min_peers, out.data_ptr() + 4 * PAD, be._stream_handle)
    assert rc == 0, be.lib.nvrx_last_error()
    be.synchronize()
    torch.cuda.synchronize()
    host = out.cpu().numpy().view(np.uint32)
    assert (host[:PAD] == FILL).all() and (host[PAD + words :] == FILL).all(), "a word outside the block changed"
    body = host[PAD : PAD + words]
    assert np.array_equal(d_groups.cpu().numpy(), np.asarray(gh, dtype=np.int32))  # the inputs are only read
    return body[: 8 * G].reshape(G, 8).copy(), body[8 * G : 264 * G].reshape(G, COLS, 4).copy(), body[264 * G :].reshape(R, 8).copy()


def _compare(got, exp, tag, exact=False):
    (gg, gp, gr), (eg, ep, er) = got, exp
    assert gg.shape == eg.shape and gp.shape == ep.shape and gr.shape == er.shape, tag
    assert np.array_equal(gp, ep), (tag, "pairs", np.argwhere(gp != ep)[:8].tolist())
    assert np.array_equal(gr[:, 4:], er[:, 4:]), (tag, "rank counts and group ids", np.argwhere(gr[:, 4:] != er[:, 4:])[:8].tolist())
    assert np.array_equal(gg[:, 2:], eg[:, 2:]), (tag, "group counts", gg[:, 2:].tolist(), eg[:, 2:].tolist())
    if exact:
        assert np.array_equal(gr, er) and np.array_equal(gg, eg), (tag, "exact", np.argwhere(gr != er)[:8].tolist())
        return 0.0
    worst = 0.0
    for what, g, e in (("ranks", gr[:, :4], er[:, :4]), ("groups", gg[:, :2], eg[:, :2])):
        g, e = np.ascontiguousarray(g).view(np.float32).astype(np.float64), np.ascontiguousarray(e).view(np.float32).astype(np.float64)
        assert np.array_equal(np.isnan(g), np.isnan(e)), (tag, what, "NaN masks", np.argwhere(np.isnan(g) != np.isnan(e))[:8].tolist())
        assert np.array_equal(np.isposinf(g), np.isposinf(e)) and np.array_equal(np.isneginf(g), np.isneginf(e)), (tag, what, "inf masks")
        fin = np.isfinite(e)
        if fin.any():
            err = float((np.abs(g[fin] - e[fin]) / np.maximum(1.0, np.abs(e[fin]))).max())
            print(tag, what, "max error", err)
            worst = max(worst, err)
            assert err <= 2e-6, (tag, what, err)
    return worst


# ---- 1. nvrx_slack_group_score against the restatement ------------------------------------------------------------------------
@pytest.mark.parametrize("R,kind", SHAPES)
def test_score_step_matches_the_restatement(be, R, kind):
    S = 2
    labels = _labels(kind, R)
    gh, G = groups_array(labels)
    max_group = int(np.bincount(labels).max())
    for K in (0, 5):
        rng = np.random.default_rng(1000 * R + 10 * K + G)
        slack, T = _slack_table(rng, R, False), random_table(rng, R, K, S)
        for min_ranks in (1, 4):
            for min_peers in (1, 2):
                exp = slack_group_records(slack, T, K, S, gh, G, max_group, min_ranks, min_peers)
                got = _run(be, slack, T, K, S, gh, G, max_group, min_ranks, min_peers)
                _compare(got, exp, (R, kind, K, min_ranks, min_peers))
                assert np.array_equal(exp[2][:, 7].view(np.int32), np.asarray(labels)) and (exp[0][:, 4] == np.bincount(labels)).all()
                if kind == "singletons" and min_peers == 2:  # every rank has collective rows and no peer: unrated
                    assert (got[2][:, 5] == 0).all() and (got[2][:, 6] > 0).all() and (got[2][:, :4] == NAN_BITS).all()
                    assert (got[1][:, :, 2].view(np.int32) == -1).all() and (got[0][:, :4] == [NAN_BITS, NAN_BITS, 0, 0]).all()
                if kind == "singletons" and min_peers == 1:  # alone and rated against itself: waits 0
                    assert (got[2][:, 5] > 0).all() and (got[0][:, 2] == 1).all()
    # sparse rows: pairs go unreferenced and ranks are left without data
    rng = np.random.default_rng(7 * R + G)
    slack, T = _slack_table(rng, R, True), random_table(rng, R, 5, S)
    _compare(_run(be, slack, T, 5, S, gh, G, max_group, 4, 2), slack_group_records(slack, T, 5, S, gh, G, max_group, 4, 2),
             (R, kind, "sparse"))


@pytest.mark.parametrize("R,kind", [(8, "2+6"), (64, "one"), (66, "65+1"), (130, "64+65+1"), (1026, "1025+1")])
def test_exact_inputs_give_exact_records(be, R, kind):
    rng = np.random.default_rng(R)
    labels = _labels(kind, R)
    gh, G = groups_array(labels)
    max_group = int(np.bincount(labels).max())
    slack = _exact_table(rng, R)
    T = random_table(rng, R, 5, 2)
    T[:, 2 * 7 : 2 * 7 + 5] = rng.integers(0, 1 << 20, (R, 5)).astype(np.float32)  # integer weights: the compute sum is exact too
    for min_ranks, min_peers in ((1, 1), (4, 2)):
        _compare(_run(be, slack, T, 5, 2, gh, G, max_group, min_ranks, min_peers),
                 slack_group_records(slack, T, 5, 2, gh, G, max_group, min_ranks, min_peers), (R, kind, min_ranks, "exact"), exact=True)


@pytest.mark.parametrize("R,kind,larger", BOTH)
def test_every_variant_of_the_group_kernel_gives_the_same_words(be, R, kind, larger):
    """``max_group`` is a promise that selects the variant; a larger value than needed is legal and selects a larger one."""
    rng = np.random.default_rng(3 * R)
    labels = _labels(kind, R)
    gh, G = groups_array(labels)
    true_max = int(np.bincount(labels).max())
    assert true_max <= 64 < larger <= R
    slack, T = _slack_table(rng, R, False), random_table(rng, R, 5, 2)
    for min_ranks, min_peers in ((1, 1), (4, 2)):
        small = _run(be, slack, T, 5, 2, gh, G, true_max, min_ranks, min_peers)
        large = _run(be, slack, T, 5, 2, gh, G, larger, min_ranks, min_peers)
        for a, b in zip(small, large):
            assert np.array_equal(a, b), (R, kind, np.argwhere(a != b)[:8].tolist())
        _compare(small, slack_group_records(slack, T, 5, 2, gh, G, true_max, min_ranks, min_peers), (R, kind, "both"))


# ---- 2. one group of all ranks is the job-wide rule ---------------------------------------------------------------------------
@pytest.mark.parametrize("R", [8, 64, 66, 1026])
def test_one_group_of_all_ranks_gives_the_job_wide_records(be, R):
    gh, G = groups_array([0] * R)
    for exact in (False, True):
        rng = np.random.default_rng(R + exact)
        slack = _exact_table(rng, R) if exact else _slack_table(rng, R, False)
        T = random_table(rng, R, 5, 2)
        if exact:
            T[:, 2 * 7 : 2 * 7 + 5] = rng.integers(0, 1 << 20, (R, 5)).astype(np.float32)
        for min_ranks in (1, 4):
            ws = be.workspace(R, 5, 2, R, 0)
            ws.slack_settle()
            ws.send.copy_(torch.from_numpy(T))
            _, table, _ = ws.slack_buffers()
            table.copy_(torch.from_numpy(slack.reshape(R, 2 * COLS)))
            torch.cuda.synchronize()
            job, cols, ranks = be.slack_score(ws, table, ws.send, 0, R, min_ranks).records()
            groups, pairs, granks = _run(be, slack, T, 5, 2, gh, G, R, min_ranks, 1)
            assert np.array_equal(pairs[0][:, :2], cols[:, :2]), (R, exact, min_ranks)
            head = np.concatenate((job[:4], np.zeros(4, dtype=np.uint32)))[None, :]
            mine = groups.copy()
            mine[:, 4:] = 0  # (the group record's fifth word is the group's size; the job record has none)
            _compare((mine, pairs[:, :, :2], granks[:, :6]), (head, cols[None, :, :2], ranks[:, :6]), (R, exact, min_ranks, "job-wide"),
                     exact=exact)
            if exact:
                ej, ec, er = slack_records(slack, T, 5, 2, min_ranks)
                assert np.array_equal(granks[:, :6], er[:, :6]) and np.array_equal(groups[0, :4], ej[:4])


# ---- 3. d_groups is data ------------------------------------------------------------------------------------------------------
def test_out_of_range_group_contents_are_guarded(be):
    """Group ids outside [0, G), members outside [0, R), ``start`` words negative, decreasing and beyond R, and a stretch above
    ``max_group``: the result is what the restatement says, and no word outside NVRX_SLACK_GROUP_WORDS of a guard-padded buffer
    is touched (``_run`` checks the guards).  Valid launches only: the kernels' guards keep every access inside the inputs and
    the buffer."""
    rng = np.random.default_rng(79)
    # the one-wave group kernel (groups of 5 or 6, once cut to 4), and the 256-thread one (groups of 66 and 4, cut to 65)
    for R, labels, largest in ((21, [r % 4 for r in range(21)], 6), (21, [r % 4 for r in range(21)], 4),
                               (70, [1 if r % 17 == 3 else 0 for r in range(70)], 65)):
        good, G = groups_array(labels)
        slack, T = _slack_table(rng, R, False), random_table(rng, R, 5, 2)
        cases = {"intact": good.copy()}
        a = cases["group id G and -1"] = good.copy()
        a[3], a[8] = G, -1
        a = cases["member R and -1"] = good.copy()
        a[R + 2], a[R + 9] = R, -1
        a = cases["start beyond R"] = good.copy()
        a[2 * R + G] = R + 5
        a = cases["start below 0 and descending"] = good.copy()
        a[2 * R], a[2 * R + 1] = -3, 0
        if G > 2:
            a[2 * R + 2] = 1
        a = cases["everything"] = good.copy()
        a[0], a[R + R - 1], a[2 * R + G], a[2 * R + 1] = G + 7, 1 << 30, 1 << 30, -(1 << 30)
        for name, arrays in cases.items():
            got = _run(be, slack, T, 5, 2, arrays, G, largest, 4, 2)
            _compare(got, slack_group_records(slack, T, 5, 2, arrays, G, largest, 4, 2), (R, largest, name))
            if name == "group id G and -1":
                assert (got[2][[3, 8], 7].view(np.int32) == -1).all() and (got[2][[3, 8], :4] == NAN_BITS).all()
                assert (got[2][[3, 8], 5] == 0).all() and (got[2][[3, 8], 6] > 0).all() and got[2][4, 5] > 0
            if name == "intact":
                assert int(got[1][0, :, 1].max()) <= largest and (got[0][:, 4] <= largest).all()  # a stretch above max_group is cut


# ---- 4. ranks without data and a slice of the ranks, through the backend -------------------------------------------------------
def test_score_step_on_ranks_without_data_and_a_slice_of_the_ranks(be):
    from nvrx_straggler.backend import PeerGroups

    rng = np.random.default_rng(5)
    for R, kind in ((8, "2+6"), (130, "64+65+1"), (1026, "1025+1")):
        labels = _labels(kind, R)
        groups = PeerGroups(labels)
        slack = _slack_table(rng, R, True)
        slack[::3, 0, :], slack[::3, 1, :] = -1.0, 0.0  # every third rank holds nothing at all
        T = random_table(rng, R, 5, 2)
        exp = slack_group_records(slack, T, 5, 2, groups.host, groups.G, groups.max_size, 4, 2)
        assert (exp[2][::3, :4] == NAN_BITS).all() and not exp[2][::3, 4:7].any()
        for lo, n in ((0, R), (R // 2, R - R // 2 - 1)):
            ws = be.workspace(R, 5, 2, R, 0)
            ws.slack_settle()
            ws.send.copy_(torch.from_numpy(T))
            _, table, _ = ws.slack_buffers()
            table.copy_(torch.from_numpy(slack.reshape(R, 2 * COLS)))
            torch.cuda.synchronize()
            handle = be.slack_group_score(ws, table, ws.send, groups, lo, n, 4, 2)
            got = handle.records()
            assert got[2].shape == (n, 8) and got[0].shape == (groups.G, 8) and got[1].shape == (groups.G, COLS, 4)
            _compare(got, (exp[0], exp[1], exp[2][lo : lo + n]), (R, kind, lo, n))
            assert ws.slack_buffers()[2].numel() >= 264 * groups.G + 8 * R
            ws.slack_settle()


# ---- 5. the step of a report ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", [TWO_SIX, "auto"], ids=["labels", "auto"])
@pytest.mark.parametrize("asynchronous", [False, True])
def test_the_step_names_the_late_host_stepwise_and_one_call(be, asynchronous, spec):
    """The 2 + 6 scenario with rank 5 late: the option names rank 5, the job-wide rule names ranks 0 and 1 in the same process,
    and the report's own scores are the same either way."""
    seen = {}
    for on, want in ((True, [5]), (False, [0, 1])):
        stats, planned = [], []
        reports = play_stages(be, TWO_SIX, 5, reports=3, peer_groups=spec, slack_peer_groups=on, asynchronous=asynchronous,
                              stats_out=stats, planned_out=planned)
        assert planned == [False, True, True]  # the stepwise path, then the one-call report
        for i, rep in enumerate(reports):
            s = rep.slack_scores()
            assert named(rep.identify_slack_stragglers()) == want, (on, i, s)
            assert bool(s.get("peer_groups")) == on and sorted(s["ranks"]) == list(range(RANKS))
            seen[on, i] = (repr(rep.gpu_relative_perf_scores), repr(rep.section_relative_perf_scores))
            if on:
                labels = (0, 2) if spec == "auto" else (0, 1)  # (inferred groups are named by their lowest rank)
                assert s["groups"] == {labels[0]: [0, 1], labels[1]: [2, 3, 4, 5, 6, 7]} and s["unrated_ranks"] == []
                g0, g1 = s["per_group"][labels[0]], s["per_group"][labels[1]]
                assert g0["typical_waited_us"] == 0.0 and abs(g1["typical_share"] - 0.156) <= 0.002 and g1["ranks_with_data"] == 6
                assert s["ranks"][5]["waited_us"] <= 3.0 * 200 and s["ranks"][5]["group"] == labels[1]
                assert all(296.0 * 200 <= s["ranks"][r]["waited_us"] <= 304.0 * 200 for r in (2, 3, 4, 6, 7))
                assert g1["columns"][column_of(ALLREDUCE)]["floor_rank"] == 5 and sorted(g1["columns"]) == sorted(
                    {column_of(ALLREDUCE), column_of(SENDRECV)})
            else:
                assert "per_group" not in s and s["typical_share"] >= 0.05 and s["ranks_with_data"] == RANKS
    for i in range(3):
        assert seen[True, i] == seen[False, i], i


def test_statistics_and_table_are_the_same_bytes_with_the_option_on_and_off(be):
    from nvrx_straggler.reporting import ReportGenerator
    from slack_group_oracle_backend import stage_scenario
    from slack_oracle_backend import GEMM

    step, gemm, allreduce, bubble = stage_scenario(TWO_SIX, 5)
    seen = {}
    for on in (True, False):
        gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=True, node_name="n", collective_slack=True,
                              peer_groups=TWO_SIX, slack_peer_groups=on)
        rings = be.make_rings(RANKS, 4, 256)
        try:
            srows = {"step": rings.row_for(0, "step")}
            krows = {GEMM: rings.row_for(1, GEMM)}  # (the collectives are in the rings' table only: the second report is the one-call one)
            rings.row_for(1, ALLREDUCE)
            rings.row_for(1, SENDRECV)
            for i in range(2):  # (stepwise, then one-call)
                for lr in range(RANKS):
                    rings.push_many(0, step[lr], lr=lr)
                    rings.push_many(1, gemm, lr=lr)
                    rings.push_many(2, allreduce[lr], lr=lr)
                    rings.push_many(3, bubble[lr], lr=lr)
                rep = gen.generate_report_from_rings(rings, srows, krows, local_ranks=RANKS)
                rings.reset()
                ws = gen._ring_plan.ws
                assert named(rep.identify_slack_stragglers()) == ([5] if on else [0, 1]) and gen._last_plan_fused == (i == 1)
                be.synchronize()
                slack_rows = ws.slack_buffers()[1].cpu().numpy().tobytes()  # the gathered rows: nothing new goes on the wire
                seen[on, i] = (ws.stats_dev.cpu().numpy().tobytes(), ws.table.cpu().numpy().tobytes(), slack_rows,
                               dict(rep.gpu_relative_perf_scores), repr(rep.local_kernel_summaries), repr(rep.peer_scores()))
        finally:
            gen.close()
            rings.close()
    for i in range(2):
        assert seen[True, i] == seen[False, i], i


@pytest.mark.parametrize("gather_on_rank0", [True, False])
def test_three_processes_sharing_the_gpu(gather_on_rank0):
    """Three gloo processes with two logical ranks each, stages of 2 and 4, rank 4 late: at most 3 processes have the GPU open."""
    import slack_group_workers
    from mp_util import run_ranks

    res = run_ranks(slack_group_workers.gpu_stage_ranks, 3, timeout=240, use_oracle_backend=False, device=0,
                    gather_on_rank0=gather_on_rank0)  # (returning at all: every rank finished)
    for r, reports in enumerate(res):
        for entry in reports:
            if gather_on_rank0 and r != 0:
                assert not entry["held"]
                continue
            s = entry["slack"]
            assert s["groups"] == {0: [0, 1], 1: [2, 3, 4, 5]} and s["peer_groups"] is True
            assert sorted(s["ranks"]) == (list(range(6)) if gather_on_rank0 else [2 * r, 2 * r + 1])
            # a report names among the ranks it covers: rank 0's with the gather, the process holding rank 4 without
            assert entry["named"] == ([4] if (gather_on_rank0 or r == 2) else []), (r, entry)
            # (a group of two: the smaller of two waits, each rank being above the other in one of the two collectives)
            assert s["per_group"][0]["typical_waited_us"] <= 25.0 * 200 and s["per_group"][1]["ranks_with_data"] == 4
            assert 290.0 * 200 <= s["per_group"][1]["typical_waited_us"] <= 310.0 * 200
            if 4 in s["ranks"]:
                assert s["ranks"][4]["waited_us"] <= 3.0 * 200


def test_the_example_names_rank_5_only_with_the_option_on():
    out = subprocess.run([sys.executable, os.path.join(REPO, "examples", "straggler_example.py"), "--slack-peer"],
                         capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    off = re.search(r"identify_slack_stragglers\(\) with slack_peer_groups=False: (\[[^\]]*\])", out.stdout)
    on = re.search(r"identify_slack_stragglers\(\) with slack_peer_groups=True: (\[[^\]]*\])", out.stdout)
    assert off and on and off.group(1) == "[0, 1]" and on.group(1) == "[5]", out.stdout
