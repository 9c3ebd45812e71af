"""Every option in ONE report on the HIP engine: the job of tests/full_report_script.py (8 folded ranks in two pipeline stages,
all follow-up results switched on, six windows) against the composed CPU checker (``full_oracle_backend.FullOracleBackend``)
and against the engine itself.

Engine against checker: every feature under the bound its own GPU file uses, imported from there, none restated --
tests/test_gpu_robust.py, test_gpu_peer.py, test_gpu_pace_group.py, test_gpu_node.py, test_gpu_slack_group.py and
test_gpu_attribution.py's ``_compare`` on the raw records, tests/test_gpu_row_group.py's ``_check_on`` on the families' dicts,
and for the scores, both histories, their trends and the work groups the rule of tests/test_gpu_score.py, test_gpu_history.py,
test_gpu_trend.py, test_gpu_peer_history.py and test_gpu_work.py: equal, the f64 weighted mean of a GPU slot (and what is
derived from it) within 2e-6 * max(1, |expected|).

Engine composed against engine alone: bit for bit.  Every kernel here reduces in a fixed order (integer LDS atomics only, no
floating-point atomics), so a word that differs means a buffer was shared, resized or read at the wrong time -- the hazards
between steps that the checker, which has no buffers and no streams, cannot have."""
import numpy as np
import pytest

import full_report_script as fs
import full_report_workers
import test_gpu_attribution as attribution
import test_gpu_node as node
import test_gpu_pace_group as pace_group
import test_gpu_peer as peer
import test_gpu_robust as robust
import test_gpu_row_group as row_group
import test_gpu_slack_group as slack_group
from full_oracle_backend import FullOracleBackend
from mp_util import run_ranks
from node_oracle_backend import node_scores_table
from pace_group_oracle_backend import pace_group_scores_table
from slack_group_oracle_backend import slack_group_records

pytestmark = pytest.mark.gpu

W = fs.WINDOWS
SUBSET = ("scores", "robust", "tail", "history", "slack")  # the second generator on the cached workspace
UNIQUE_ROWS = fs.ROWS_PER_RANK + 1  # a workspace shape no other test of the session uses (the cache is per shape)


@pytest.fixture(scope="module")
def be():
    from nvrx_straggler.backend import get_backend

    return get_backend()


def _take(job, rep, features=None):
    """What one report holds: the raw records (before the readers materialise them), the readers' dicts, who is named."""
    return {"raw": fs.raw(rep, features), "read": fs.read(rep, features), "identified": fs.identified(rep, features)}


def _inputs(backend_, job):
    """The inputs of the restatements for the report ``job`` issued last: the exchanged table, the resolved groups and nodes
    and -- on the engine -- the gathered slack rows [R, 2, 64].  On the engine this waits for the report's kernels (their
    buffers stay as they are until the next report); the report itself stays unread."""
    ws, gen = job.gen._ring_plan.ws, job.gen
    backend_.synchronize()
    extra = {"table": ws.table.cpu().numpy().copy(), "shape": (ws.R, ws.K, ws.S)}
    if getattr(ws, "_slack_state", None) is not None:
        extra["slack"] = ws._slack_state[1].cpu().numpy().reshape(ws.R, 2, -1).copy()
    for key, g in (("groups", gen._peer_resolved), ("nodes", gen._node_resolved)):
        if g is not None:
            extra[key] = (g.host.copy(), g.G, g.max_size)
    return extra


def _play(backend_, features=None, windows=W, asynchronous=False, order="now", tables=False, **job_options):
    """``windows`` reports of one job on ``backend_``; ``order`` as tests/test_full_report_host.py spells it ("now", "late":
    newest first after the last was issued, "last": the others dropped unread).  ``tables``: also the exchanged table and
    the resolved groups of every window -- the restatements' inputs -- and, on the engine, the gathered slack rows."""
    job = fs.Job(backend_, features, asynchronous=asynchronous, **job_options)
    try:
        out, held = [None] * windows, []
        for w in range(windows):
            rep = job.report(w)
            if order == "now":
                out[w] = _take(job, rep, features)
            elif order == "late" or w == windows - 1:
                held.append((w, rep))
            if tables:
                out[w] = dict(out[w] or {}, **_inputs(backend_, job))
            del rep
        for w, rep in reversed(held):
            out[w] = dict(out[w] or {}, **_take(job, rep, features))
        return out
    finally:
        job.close()


@pytest.fixture(scope="module")
def checker():
    """The reference, computed once on the composed CPU checker and left unchanged: the composed job, the job whose inferred
    groups change, the 66-rank job and the second generator's subset."""
    from nvrx_straggler import backend

    before = backend._backend

    def on_checker(**kw):
        cpu = FullOracleBackend(emulate_fused=True)
        backend.set_backend(cpu)
        return _play(cpu, tables=True, **kw)

    try:
        return {"composed": on_checker(), "variant": on_checker(variant=True, peer_groups="auto"),
                "wide": on_checker(windows=2, ranks=66), "subset": on_checker(features=SUBSET, windows=3)}
    finally:
        backend.set_backend(before)


def _near(a, b) -> bool:
    """``fs.same``, a float within 2e-6 * max(1, |expected|) of the expected one (the bound of the f64 weighted mean behind a
    GPU slot, tests/test_gpu_score.py; NaN equal to NaN, infinities equal)."""
    if isinstance(a, dict) and isinstance(b, dict):
        return a.keys() == b.keys() and all(_near(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        return len(a) == len(b) and all(_near(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and isinstance(b, float):
        return (a != a and b != b) or a == b or (np.isfinite(a) and np.isfinite(b) and abs(a - b) <= 2e-6 * max(1.0, abs(b)))
    return fs.same(a, b)


def _sections_same(got, want) -> bool:
    """The ``section_*`` parts of a reader's dict: one f64 quotient rounded to f32 each, equal to the bit."""
    if isinstance(got, dict) and isinstance(want, dict):
        return all(fs.same(got[k], want[k]) if str(k).startswith("section_") else _sections_same(got[k], want[k])
                   for k in want if k in got)
    return True


def _check(got, want, tag, features=None):
    """One engine report against the checker's report of the same window, feature by feature."""
    features = fs.FEATURES if features is None else features
    R, K, S = want["shape"]
    graw, wraw = got["raw"], want["raw"]
    for feature in features:
        where = tag + (feature,)
        g, w = got["read"][feature], want["read"][feature]
        if feature == "attribution":
            attribution._compare(graw[feature][0], wraw[feature][0], where)
        elif feature == "robust":
            robust._compare(tuple(graw[feature]), tuple(wraw[feature]), where)
        elif feature == "peer":
            peer._compare(tuple(graw[feature]), tuple(wraw[feature]), where)
        elif feature == "pace":
            host, G, largest = want["groups"]
            exp = pace_group_scores_table(want["table"], K, S, host, G, largest, 0, R, min(4, R), 2)
            assert all(np.array_equal(a, b) for a, b in zip(exp[:2], wraw[feature])), where  # (the checker IS the restatement)
            pace_group._compare(tuple(graw[feature]), exp, where)
        elif feature == "node":
            host, G, largest = want["nodes"]
            exp = node_scores_table(want["table"], K, S, host, G, largest, 2, min(3, G), 0, R)
            assert all(np.array_equal(a, b) for a, b in zip(exp[:4], wraw[feature])), where
            node._compare(tuple(graw[feature]), exp, where)
        elif feature == "slack":
            # the step's inputs are sums of the statistics kernel's means, which the engine and the checker add up in another
            # order: against the checker the counts are equal and the sums within tests/test_gpu_slack.py's 2e-6; the
            # records are held to tests/test_gpu_slack_group.py's rule against the restatement on the ENGINE's own inputs
            assert g.keys() == w.keys() and fs.same(g["groups"], w["groups"]) and sorted(g["ranks"]) == sorted(w["ranks"]), where
            assert {c: sorted(v["columns"]) for c, v in g["per_group"].items()} == {c: sorted(v["columns"]) for c, v in w["per_group"].items()}
            for r, rec in w["ranks"].items():
                assert g["ranks"][r]["calls"] == rec["calls"] and g["ranks"][r]["group"] == rec["group"], (where, r)
                for key in ("collective_us", "compute_us"):
                    assert abs(g["ranks"][r][key] - rec[key]) <= 2e-6 * rec[key], (where, r, key, g["ranks"][r][key], rec[key])
            assert "slack" in got, (where, "the engine run was played without its inputs (_inputs)")
            host, G, largest = want["groups"]
            assert np.array_equal(got["groups"][0], host) and got["groups"][1:] == (G, largest), where
            exp = slack_group_records(got["slack"], got["table"], K, S, host, G, largest, 4, 2)
            slack_group._compare(tuple(graw[feature]), exp, where)
        elif feature == "work":
            assert all(np.array_equal(a, b) for a, b in zip(graw[feature], wraw[feature])) and fs.same(g, w), (where, g, w)
        elif feature in fs.FAMILY_NAMES:
            continue  # (all four together, below)
        else:  # scores, history, peer_history
            # the raw history and trend records [ranks, families, 1 + S, words]: the section columns are equal word for word,
            # as tests/test_gpu_history.py, test_gpu_trend.py and test_gpu_peer_history.py compare them; column 0 -- the GPU
            # slot, an f64 weighted mean summed in another order -- and what the readers derive from it within _near's bound
            for i, (a, b) in enumerate(zip(graw.get(feature, ()), wraw.get(feature, ()))):
                a, b = a.view(np.uint32), b.view(np.uint32)
                assert a.shape == b.shape and a.ndim == 4 and a.shape[2] == 1 + S, (where, i, a.shape, b.shape)
                assert np.array_equal(a[:, :, 1:], b[:, :, 1:]), (where, i, np.argwhere(a[:, :, 1:] != b[:, :, 1:])[:8].tolist())
            assert (feature == "scores") == (feature not in graw) and len(graw.get(feature, ())) == len(wraw.get(feature, ()))
            assert _sections_same(g, w) and _near(g, w), (where, g, w)
    fams = [f for f in fs.FAMILY_NAMES if f in features]
    if len(fams) == 4:
        row_group._check_on({f: got["read"][f] for f in fams}, {f: want["read"][f] for f in fams}, tag)
    else:
        for f in fams:
            assert row_group._close(got["read"][f], want["read"][f]), (tag, f)
    assert got["identified"] == want["identified"], (tag, got["identified"], want["identified"])


# ---- 1. engine equals checker, composed ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("asynchronous", [False, True])
def test_the_composed_job_on_the_engine_equals_the_checkers(be, checker, asynchronous):
    """Six windows with everything on (the general report, then planned ones), each report read right away."""
    got = _play(be, asynchronous=asynchronous, tables=True)
    for w in range(W):
        _check(got[w], checker["composed"][w], (asynchronous, w))
    who = fs.plants()
    assert got[-1]["identified"]["identify_slack_stragglers"] == [who["late"]]
    assert got[-1]["identified"]["identify_pace_stragglers"] == [who["pace"]]


# ---- 2. engine composed equals engine alone, word for word ------------------------------------------------------------------------
def _words(value):
    """The leaves of a reader's dict as one flat list (for features without a raw handle)."""
    if isinstance(value, dict):
        return [x for k in sorted(value, key=repr) for x in [repr(k)] + _words(value[k])]
    if isinstance(value, (list, tuple)):
        return [x for v in value for x in _words(v)]
    return [np.float64(value).view(np.uint64).item() if isinstance(value, float) else value]


def test_every_feature_alone_on_the_engine_is_the_composed_run_bit_for_bit(be):
    """The raw records of the composed run (asynchronous, every report held until the last was issued) against those of a
    generator with only that feature's options, on the same engine and the same workspace: every word equal."""
    composed = _play(be, asynchronous=True, order="late")
    compared = {}
    for feature in fs.FEATURES:
        alone = _play(be, [feature], asynchronous=True, order="late")
        words = 0
        for w in range(W):
            a, c = alone[w]["raw"].get(feature), composed[w]["raw"].get(feature)
            if a is None:  # no handle behind it: the public dicts
                assert c is None and feature == "scores"
                wa, wc = _words(alone[w]["read"][feature]), _words(composed[w]["read"][feature])
                assert wa == wc, (feature, w, alone[w]["read"][feature], composed[w]["read"][feature])
                words += len(wa)
                continue
            assert len(a) == len(c), (feature, w)
            for i, (x, y) in enumerate(zip(a, c)):
                assert x.shape == y.shape and x.dtype == y.dtype, (feature, w, i, x.shape, y.shape)
                xb, yb = x.view(np.uint32), y.view(np.uint32)
                assert np.array_equal(xb, yb), (feature, w, i, np.argwhere(xb != yb)[:8].tolist())
                words += xb.size
            assert fs.same(alone[w]["read"][feature], composed[w]["read"][feature]), (feature, w)
        compared[feature] = words
    print("bit for bit:", len(compared), "features,", sum(compared.values()), "words:", compared)
    assert len(compared) == len(fs.FEATURES) and all(n > 0 for n in compared.values()), compared


# ---- 3. reading orders, and a second generator on the cached workspace --------------------------------------------------------
def test_reading_orders_and_a_second_generator_on_the_same_workspace(be, checker):
    """Asynchronous, composed: read right away; all six read newest first after the last was issued; reports 0-4 never read
    and dropped, the generator closed.  Then a second generator with a subset of the options runs three reports on the same
    cached workspace and still matches the checker."""
    now = _play(be, asynchronous=True, tables=True)
    late = _play(be, asynchronous=True, order="late", tables=True)
    for w in range(W):
        assert fs.same(late[w]["read"], now[w]["read"]) and late[w]["identified"] == now[w]["identified"], w
        _check(late[w], checker["composed"][w], ("late", w))
    job = fs.Job(be, asynchronous=True)
    try:
        for w in range(W - 1):
            job.report(w)  # never read, dropped
        rep = job.report(W - 1)
        ws = job.gen._ring_plan.ws
        last = dict(_inputs(be, job), **_take(job, rep))
    finally:
        job.close()
    assert fs.same(last["read"], now[-1]["read"]) and last["identified"] == now[-1]["identified"]
    _check(last, checker["composed"][-1], ("last",))
    job = fs.Job(be, SUBSET, asynchronous=True)
    try:
        got = []
        for w in range(3):
            rep = job.report(w)
            got.append(dict(_inputs(be, job), **_take(job, rep, SUBSET)))
        ws2 = job.gen._ring_plan.ws
    finally:
        job.close()
    assert ws2 is ws
    for w in range(3):
        _check(got[w], checker["subset"][w], ("subset", w), SUBSET)


# ---- 4. inferred groups that change, reports held ---------------------------------------------------------------------------------
def _watch(ws, held, settles, inside):
    """Spies on the workspace ``ws``: ``settles`` gets ``(reports issued so far, name, the buffer's size then)`` for every
    settle called from inside ``family_buffers`` / ``slack_buffers``."""
    inner_buffers, inner_slack = ws.family_buffers, ws.slack_buffers
    inner_fs, inner_ss = ws.family_settle, ws.slack_settle

    def family_buffers(fam, group_words=0):
        inside.append(fam.name)
        try:
            return inner_buffers(fam, group_words)
        finally:
            inside.pop()

    def slack_buffers(group_words=0):
        inside.append("slack")
        try:
            return inner_slack(group_words)
        finally:
            inside.pop()

    def family_settle(fam):
        if inside:
            settles.append((len(held), fam.name, ws._family_state[fam.name].buf.numel()))
        return inner_fs(fam)

    def slack_settle():
        if inside:
            settles.append((len(held), "slack", ws._slack_state[2].numel()))
        return inner_ss()

    ws.family_buffers, ws.slack_buffers = family_buffers, slack_buffers
    ws.family_settle, ws.slack_settle = family_settle, slack_settle


def test_inferred_groups_that_change_grow_the_buffers_behind_their_settles(be, checker):
    """The variant (rank 2 runs another GEMM in window 3 only: 2 -> 3 -> 2 groups) with ``peer_groups="auto"``, asynchronous,
    every report held: in window 3 every family's buffer and the slack step's ``out`` grow on the one workspace, and the held
    reports keep their records -- outcomes.  That each growth goes through its settle from inside the growing call is a pin
    on the implementation's SHAPE, not an outcome: in this flow ``settle_readers`` has delivered the last step at the start
    of the report, so the settle in the growth branch finds nothing to do, and dropping it changes no record -- only the
    spies below see it.  It is pinned because it is what keeps a caller outside a report (a direct ``*_group_score`` on a
    workspace with a step in flight) safe; a refactor that settles elsewhere has to move this assertion with it."""
    from nvrx_straggler import row_families

    job = fs.Job(be, asynchronous=True, variant=True, peer_groups="auto", rows_per_rank=UNIQUE_ROWS)
    settles, inside = [], []
    try:
        held, sizes, spaces, inputs = [], [], [], []
        for w in range(W):
            held.append(job.report(w))
            ws = job.gen._ring_plan.ws
            inputs.append(_inputs(be, job))
            if w == 0:  # watch the workspace from the first report on: who settles, and from where
                _watch(ws, held, settles, inside)
            spaces.append(ws)
            sizes.append({**{f.name: ws._family_state[f.name].buf.numel() for f in row_families.FAMILIES},
                          "slack": ws._slack_state[2].numel()})
        assert all(s is spaces[0] for s in spaces)
        names = [f.name for f in row_families.FAMILIES] + ["slack"]
        assert sizes[0] == sizes[1] == sizes[2] and sizes[3] == sizes[4] == sizes[5]
        assert all(sizes[3][n] > sizes[2][n] for n in names), (sizes[2], sizes[3])
        # every growth went through its settle, inside the growing call, while the buffer still had its old size
        assert sorted(settles) == sorted((3, n, sizes[2][n]) for n in names), settles
        got = [dict(inputs[w], **_take(job, rep)) for w, rep in enumerate(held)]
    finally:
        ws = job.gen._ring_plan.ws if job.gen._ring_plan is not None else None
        if ws is not None:
            for name in ("family_buffers", "slack_buffers", "family_settle", "slack_settle"):
                ws.__dict__.pop(name, None)
        job.close()
    assert [len(g["read"]["tail"]["groups"]) for g in got] == [len(g["read"]["slack"]["groups"]) for g in got] == [2, 2, 2, 3, 2, 2]
    for w in range(W):
        _check(got[w], checker["variant"][w], ("variant", w))


# ---- 5. the sizes past a wave -----------------------------------------------------------------------------------------------------
def test_sixty_six_folded_ranks_composed_on_the_engine(be, checker):
    """66 logical ranks, stages of 33: ``k_robust_cols<256>``, ``k_colmin_part`` / ``k_colmin_finish``, the tiled score route
    and ``k_slack_group_job``'s larger variant in one report; one synchronous and one asynchronous pair of reports."""
    for asynchronous in (False, True):
        got = _play(be, windows=2, asynchronous=asynchronous, order="late", tables=True, ranks=66)
        for w in range(2):
            _check(got[w], checker["wide"][w], ("wide", asynchronous, w))


# ---- 6. two processes sharing the GPU ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gather", [True, False])
def test_two_processes_sharing_the_gpu_give_the_folded_reports(be, gather):
    """Four logical ranks per process (gloo, the default route): with ``gather_on_rank0`` rank 0's reports are those of the
    folded run on the same engine and rank 1 holds none; without it either rank's reports say about its own ranks what the
    folded run says about them."""
    folded = _play(be, windows=3, order="late")
    res = run_ranks(full_report_workers.composed_reports, 2, timeout=420, use_oracle_backend=False, device=0,
                    gather_on_rank0=gather, windows=3)
    if gather:
        assert res[1]["reports"] == [None] * 3
        for w, got in enumerate(res[0]["reports"]):
            for feature in fs.FEATURES:
                assert fs.same(got["read"][feature], folded[w]["read"][feature]), (w, feature, got["read"][feature], folded[w]["read"][feature])
            assert got["identified"] == folded[w]["identified"], w
        return
    for rank in (0, 1):
        own = range(4 * rank, 4 * rank + 4)
        for w, got in enumerate(res[rank]["reports"]):
            for feature in fs.FEATURES:
                mine, want = fs.per_rank(got["read"][feature]), fs.per_rank(folded[w]["read"][feature], own)
                assert mine and fs.same(mine, want), (rank, w, feature, mine, want)
