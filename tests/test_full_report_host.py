"""Every option in ONE report on a box without a GPU: the job of tests/full_report_script.py on the composed checker
(``full_oracle_backend.FullOracleBackend``).  The checker has no buffers and no streams, so what these tests hold still is the
host side of the composition: every feature says composed what it says alone, in any reading order, every step runs once per
report, inferred groups agree with the labels and survive a change, the sizes past a wave are taken, and every rank of a
two-process job issues the same collectives.  The same script runs on the HIP engine in tests/test_gpu_full_report.py."""
import math

import pytest

import full_report_script as fs
import full_report_workers
import mp_util
from full_oracle_backend import FullOracleBackend

COMBOS = [(False, False), (True, False), (True, True)]  # (emulate_fused, asynchronous), as tests/test_slack_host.py
W = fs.WINDOWS


def _play(features=None, windows=W, emulate_fused=False, asynchronous=False, order="now", **job_options):
    """One job on a checker of its own: ``([what fs.read says per window], [who is named per window], backend, job)``,
    the job closed.  ``order``: "now" reads each report right away, "late" all of them newest first after the last was
    issued, "last" drops the others unread and reads the last only (their entries are None)."""
    from nvrx_straggler import backend

    be = FullOracleBackend(emulate_fused=emulate_fused)
    backend.set_backend(be)
    job = fs.Job(be, features, asynchronous=asynchronous, **job_options)
    try:
        said, named = [None] * windows, [None] * windows

        def take(w, rep):
            said[w], named[w] = fs.read(rep, features), fs.identified(rep, features)

        held = []
        for w in range(windows):
            rep = job.report(w)
            if order == "now":
                take(w, rep)
            elif order == "late" or w == windows - 1:
                held.append((w, rep))
            del rep
        for w, rep in reversed(held):
            take(w, rep)
        return said, named, be, job
    finally:
        job.close()
        backend.set_backend(None)


_COMPOSED = {}


def _composed(emulate_fused, asynchronous):
    """The composed job read right away, once per mode."""
    key = (emulate_fused, asynchronous)
    if key not in _COMPOSED:
        _COMPOSED[key] = _play(emulate_fused=emulate_fused, asynchronous=asynchronous)
    return _COMPOSED[key]


def _floats(value, under, named=None):
    """The float leaves of ``value`` below the top-level keys ``under`` (whose own key is in ``named``, if given)."""
    out = []

    def walk(v, key):
        if isinstance(v, dict):
            for k, x in v.items():
                walk(x, k)
        elif isinstance(v, (list, tuple)):
            for x in v:
                walk(x, key)
        elif isinstance(v, float) and (named is None or key in named):
            out.append(v)

    for k in under:
        walk(value[k], k)
    return out


# where each feature's scores live in what its reader returns: (top-level keys, leaf keys or None for all)
LIVE = {
    "scores": (("gpu_relative", "section_relative"), None),
    "attribution": (("relative",), ("deficit", "share", "score")),
    "robust": (("gpu_z", "section_z", "gpu_ratio", "section_ratio"), None),
    "tail": (("gpu_relative", "section_relative"), None), "onset": (("gpu_relative", "section_relative"), None),
    "period": (("gpu_relative", "section_relative"), None), "episode": (("gpu_relative", "section_relative"), None),
    "peer": (("gpu_relative", "section_relative"), None),
    "peer_history": (("history", "trends"), ("latest", "worst", "slope")),
    "pace": (("ranks",), ("pace",)), "node": (("node_scores", "ranks"), ("pace",)),
    "history": (("history", "trends"), ("latest", "worst", "slope")),
    "slack": (("ranks",), ("waited_us", "share")),
}


# ---- 1. the composition itself ------------------------------------------------------------------------------------------------
def test_the_composed_checker_is_both_parents_on_one_chain():
    from row_group_oracle_backend import RowGroupOracleBackend
    from slack_group_oracle_backend import SlackGroupOracleBackend

    be = FullOracleBackend(emulate_fused=True)
    assert be.emulate_fused is True and isinstance(be, RowGroupOracleBackend) and isinstance(be, SlackGroupOracleBackend)
    assert be.row_group_calls == [] and be.slack_group_calls == 0 and be.peer_history_calls == 0  # both parents' counters
    assert all(hasattr(be, name) for name in ("tail_group_score", "onset_group_score", "period_group_score",
                                              "episode_group_score", "slack_group_score", "peer_history", "work_groups",
                                              "node_score", "pace_group_score", "peer_score", "score_trend", "attribute"))
    assert not hasattr(RowGroupOracleBackend(), "slack_group_score") and not hasattr(SlackGroupOracleBackend(), "tail_group_score")
    assert set(fs.options_of()) >= {"kernel_attribution", "robust_scores", "tail_quantile", "onset_detection", "period_detection",
                                    "episode_detection", "row_peer_groups", "peer_history", "peer_trends", "pace_scores",
                                    "pace_peer_groups", "node_scores", "score_history", "score_trends", "collective_slack",
                                    "slack_peer_groups", "work_groups", "peer_groups", "node_groups"}


def test_no_comparison_is_vacuous():
    """The composed report of the last window: every feature has a value that is neither NaN nor neutral (1.0 for a ratio, 0.0
    for a z, a wait or a slope), and every ``identify_*`` the plants are meant for names somebody and not everybody."""
    said, named, _, _ = _composed(True, True)
    last, who = said[-1], fs.plants()
    assert set(LIVE) | {"work"} == set(fs.FEATURES)
    for feature, (under, leaves) in LIVE.items():
        values = _floats(last[feature], under, leaves)
        assert any(not math.isnan(v) and v not in (0.0, 1.0) for v in values), (feature, values)
    work = last["work"]
    assert work["groups"] == {0: [0, 1, 2, 3], 4: [4, 5, 6, 7]} and work["label_conflicts"] == {}
    for method, ranks in named[-1].items():
        assert ranks and len(ranks) < fs.RANKS, (method, ranks)
    got = named[-1]
    assert got["identify_slack_stragglers"] == [who["late"]] and got["identify_pace_stragglers"] == [who["pace"]]
    assert got["identify_onset_stragglers"] == [who["onset"]] and got["identify_period_stragglers"] == [who["beat"]]
    assert who["stretch"] in got["identify_episode_stragglers"] and who["tail"] in got["identify_tail_stragglers"]
    assert got["identify_persistent_stragglers"] == got["identify_persistent_peer_stragglers"] == [who["history"]]
    assert who["drift"] in got["identify_declining_stragglers"] and who["drift"] in got["identify_declining_peer_stragglers"]
    assert who["pace"] in got["identify_robust_stragglers"] and who["history"] in got["identify_peer_stragglers"]
    # the wrapped ring, in time order: the step of the onset rank lies 64 samples back in a window of 256
    rec = last["onset"]["section_onsets"]["step"][who["onset"]]
    assert rec["samples_ago"] == 64 and rec["window"] == fs.RING_CAP
    assert named[0]["identify_persistent_stragglers"] == [] and named[2]["identify_declining_stragglers"] == []  # (minimums not reached)


@pytest.mark.parametrize("emulate_fused,asynchronous", COMBOS)
def test_every_feature_says_composed_what_it_says_alone(emulate_fused, asynchronous):
    """For every entry of ``FEATURES``: the six composed reports say exactly (``same``: NaN equal to NaN) what six reports of a
    generator with only that feature's options say, on the same pushes.  One exception by design: ``work_groups()`` gains the
    labelled comparison when ``peer_groups`` labels are set (``ReportGenerator._follow_ups``), so "alone" for it is
    ``work_groups=True`` WITH the labels (``FEATURES["work"]``), not ``work_groups=True`` alone -- which differs, as asserted."""
    composed, composed_named, _, _ = _composed(emulate_fused, asynchronous)
    for feature in fs.FEATURES:
        alone, alone_named, _, _ = _play([feature], emulate_fused=emulate_fused, asynchronous=asynchronous)
        for w in range(W):
            assert fs.same(composed[w][feature], alone[w][feature]), (feature, w, composed[w][feature], alone[w][feature])
            for method in fs.IDENTIFY.get(feature, ()):
                assert composed_named[w][method] == alone_named[w][method], (feature, w, method)
    from nvrx_straggler import backend

    be = FullOracleBackend(emulate_fused=emulate_fused)
    backend.set_backend(be)
    try:
        job = fs.Job(be, ["scores"], asynchronous=asynchronous, work_groups=True)
        unlabelled = job.report(0).work_groups()
        job.close()
    finally:
        backend.set_backend(None)
    assert "label_conflicts" not in unlabelled and "label_conflicts" in composed[0]["work"]
    assert {k: v for k, v in composed[0]["work"].items() if k != "label_conflicts"} == unlabelled


@pytest.mark.parametrize("emulate_fused,asynchronous", COMBOS)
def test_the_reading_order_changes_nothing(emulate_fused, asynchronous):
    now, now_named, _, _ = _composed(emulate_fused, asynchronous)
    late, late_named, _, _ = _play(emulate_fused=emulate_fused, asynchronous=asynchronous, order="late")
    last, last_named, _, _ = _play(emulate_fused=emulate_fused, asynchronous=asynchronous, order="last")
    for w in range(W):
        assert fs.same(late[w], now[w]) and late_named[w] == now_named[w], w
    assert last[:-1] == [None] * (W - 1) and fs.same(last[-1], now[-1]) and last_named[-1] == now_named[-1]


# ---- 2. every step once per report -------------------------------------------------------------------------------------------
ONCE = ("score_calls", "tail_local_calls", "onset_local_calls", "period_local_calls", "episode_local_calls", "attribute_calls",
        "robust_calls", "history_calls", "trend_calls", "slack_local_calls", "peer_calls", "pace_group_calls", "node_calls",
        "work_calls", "peer_history_calls", "peer_trend_calls", "slack_group_calls")
NEVER = ("tail_score_calls", "onset_score_calls", "period_score_calls", "episode_score_calls", "slack_score_calls", "pace_calls")


def _counters(be):
    return {k: v for k, v in vars(be).items() if k.endswith("_calls")}


@pytest.mark.parametrize("emulate_fused,asynchronous", COMBOS)
@pytest.mark.parametrize("spec", ["labels", "auto"])
def test_every_step_runs_once_per_report(emulate_fused, asynchronous, spec):
    options = {} if spec == "labels" else {"peer_groups": "auto"}
    _, _, be, job = _play(emulate_fused=emulate_fused, asynchronous=asynchronous, order="last", **options)
    got = _counters(be)
    assert set(got) == set(ONCE) | set(NEVER) | {"row_group_calls", "onset_enable_calls"}, sorted(got)
    assert {k: got[k] for k in ONCE} == {k: W for k in ONCE} and {k: got[k] for k in NEVER} == {k: 0 for k in NEVER}
    assert got["row_group_calls"] == list(fs.FAMILY_NAMES) * W and got["onset_enable_calls"] == 1
    assert be.peer_history_grown == 0 and len(be.work_handles) == W
    if spec == "auto":
        # the work step's records are fetched for the grouped steps of every report, read or not, and the groups object was
        # built once: the roots never changed
        assert all(h.reads >= 1 for h in be.work_handles[:-1]), [h.reads for h in be.work_handles]
        assert {a[4] for a in be.row_group_args} == {2} and {a[3] for a in be.slack_group_args} == {2}
        assert job.gen._peer_auto_roots.tolist() == [0, 0, 0, 0, 4, 4, 4, 4]
    else:
        assert all(h.reads == 0 for h in be.work_handles[:-1])  # nobody waited for an unread report's work step


# ---- 3. inferred groups --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("emulate_fused,asynchronous", COMBOS)
def test_inferred_groups_say_what_the_labels_say(emulate_fused, asynchronous):
    """``peer_groups="auto"``: everything keyed by rank equals the run with the labels; what is keyed by group label is
    compared through the rank -> group map (the labels are 0 and 1, the roots 0 and 4).  ``work_groups()`` has its labelled
    comparison only with labels."""
    labelled, labelled_named, _, _ = _composed(emulate_fused, asynchronous)
    auto, auto_named, _, _ = _play(emulate_fused=emulate_fused, asynchronous=asynchronous, peer_groups="auto")
    for w in range(W):
        assert auto_named[w] == labelled_named[w], w
        want_of, got_of = labelled[w]["peer"]["group_of"], auto[w]["peer"]["group_of"]
        assert sorted(set(got_of.values())) == [0, 4] and sorted(set(want_of.values())) == [0, 1]
        for feature in fs.FEATURES:
            if feature == "work":  # (named by its own roots either way)
                want, got = dict(labelled[w][feature]), auto[w][feature]
                assert want.pop("label_conflicts") == {} and "label_conflicts" not in got
            else:
                want, got = fs.by_rank(labelled[w][feature], want_of), fs.by_rank(auto[w][feature], got_of)
            assert fs.same(got, want), (w, feature, got, want)


@pytest.mark.parametrize("emulate_fused,asynchronous", COMBOS)
def test_inferred_groups_that_change_with_earlier_reports_unread(emulate_fused, asynchronous):
    """The variant: rank 2 runs another GEMM in window 3 only, so the inferred groups go 2 -> 3 -> 2 while every report is
    held unread.  Every held report says what a fresh generator run up to that window says, and the groups object is rebuilt
    exactly when the roots change."""
    from nvrx_straggler import backend

    be = FullOracleBackend(emulate_fused=emulate_fused)
    backend.set_backend(be)
    try:
        job = fs.Job(be, asynchronous=asynchronous, variant=True, peer_groups="auto")
        held, resolved = [], []
        for w in range(W):
            held.append(job.report(w))
            resolved.append(job.gen._peer_resolved)
        assert [g.G for g in resolved] == [2, 2, 2, 3, 2, 2]
        assert resolved[0] is resolved[1] is resolved[2] and resolved[4] is resolved[5]
        assert resolved[3] is not resolved[2] and resolved[4] is not resolved[3]
        said = [fs.read(rep) for rep in held]
        job.close()
    finally:
        backend.set_backend(None)
    assert [len(s["tail"]["groups"]) for s in said] == [len(s["slack"]["groups"]) for s in said] == [2, 2, 2, 3, 2, 2]
    assert said[3]["work"]["groups"] == {0: [0, 1, 3], 2: [2], 4: [4, 5, 6, 7]} and said[3]["peer"]["unrated_ranks"] == [2]
    for w in range(W):
        fresh = _play(windows=w + 1, emulate_fused=emulate_fused, asynchronous=asynchronous, order="last", variant=True,
                      peer_groups="auto")[0][w]
        for feature in fs.FEATURES:
            assert fs.same(said[w][feature], fresh[feature]), (w, feature, said[w][feature], fresh[feature])


# ---- 4. the sizes past a wave ---------------------------------------------------------------------------------------------------
def test_sixty_six_folded_ranks_composed():
    """66 logical ranks, stages of 33: the first size past a wave, past the 64 ranks of the tiled column kernels and of the
    single-workgroup score.  Two composed reports; the plants are found where the script put them, and the features that
    take another kernel on the engine at this size say composed what they say alone."""
    ranks, who = 66, fs.plants(66)
    said, named, be, _ = _play(windows=2, emulate_fused=True, asynchronous=True, order="late", ranks=ranks)
    got = named[-1]
    assert got["identify_slack_stragglers"] == [who["late"]] and got["identify_pace_stragglers"] == [who["pace"]]
    assert got["identify_onset_stragglers"] == [who["onset"]] and got["identify_period_stragglers"] == [who["beat"]]
    assert who["stretch"] in got["identify_episode_stragglers"] and who["tail"] in got["identify_tail_stragglers"]
    assert said[-1]["work"]["groups"] == {0: list(range(33)), 33: list(range(33, 66))}
    assert {a[1] for a in be.row_group_args} == {66} and {a[0] for a in be.slack_group_args} == {66}
    assert be.slack_group_args[0][4] == 33  # (the largest group: the slack step's larger variant on the engine)
    for feature in ("robust", "slack", "tail", "scores"):
        alone = _play([feature], windows=2, emulate_fused=True, asynchronous=True, ranks=ranks)[0]
        assert all(fs.same(said[w][feature], alone[w][feature]) for w in range(2)), feature


# ---- 5. two processes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("emulate_fused,asynchronous", [(False, False), (True, True)])
def test_two_processes_that_gather_give_the_folded_reports(emulate_fused, asynchronous):
    """Four logical ranks per process, ``gather_on_rank0=True``: rank 1 returns None and still issues every collective (a rank
    left inside one shows as ``run_ranks``' timeout); rank 0's reports are the folded run's."""
    folded, folded_named, be, _ = _play(windows=3, emulate_fused=emulate_fused, asynchronous=asynchronous, order="late")
    res = mp_util.run_ranks(full_report_workers.composed_reports, 2, timeout=180, cpu=True, gather_on_rank0=True,
                            emulate_fused=emulate_fused, asynchronous=asynchronous, windows=3)
    assert res[1]["reports"] == [None] * 3
    for w, got in enumerate(res[0]["reports"]):
        for feature in fs.FEATURES:
            assert fs.same(got["read"][feature], folded[w][feature]), (w, feature, got["read"][feature], folded[w][feature])
        assert got["identified"] == folded_named[w], w
    # (the first score round of a multi-process job is repeated once after the name sync: ``ReportGenerator._score_round``)
    assert res[0]["counters"] == dict(_counters(be), score_calls=3 + 1) and res[0]["first_ranks"] == [0]
    # the rank without a report ran the local steps and the collectives, and no score step
    idle = res[1]["counters"]
    assert {idle[k] for k in ("tail_local_calls", "onset_local_calls", "period_local_calls", "episode_local_calls",
                              "slack_local_calls")} == {3}
    assert idle["row_group_calls"] == [] and idle["slack_group_calls"] == 0 and idle["peer_calls"] == 0 and res[1]["first_ranks"] == []


@pytest.mark.parametrize("emulate_fused,asynchronous", [(False, False), (True, True)])
def test_two_processes_that_do_not_gather_give_their_halves_of_the_folded_reports(emulate_fused, asynchronous):
    """``gather_on_rank0=False``: every follow-up of rank 1 runs with ``first_rank=4`` in one report; what either rank's
    reports say about its own ranks is what the folded run says about them."""
    folded, _, _, _ = _play(windows=3, emulate_fused=emulate_fused, asynchronous=asynchronous, order="late")
    res = mp_util.run_ranks(full_report_workers.composed_reports, 2, timeout=180, cpu=True, gather_on_rank0=False,
                            emulate_fused=emulate_fused, asynchronous=asynchronous, windows=3)
    for rank in (0, 1):
        own = range(4 * rank, 4 * rank + 4)
        assert res[rank]["first_ranks"] == [4 * rank]
        assert res[rank]["counters"]["row_group_calls"] == list(fs.FAMILY_NAMES) * 3 and res[rank]["counters"]["slack_group_calls"] == 3
        for w, got in enumerate(res[rank]["reports"]):
            for feature in fs.FEATURES:
                mine, want = fs.per_rank(got["read"][feature]), fs.per_rank(folded[w][feature], own)
                assert mine and fs.same(mine, want), (rank, w, feature, mine, want)
                assert all(set(m) <= set(own) for m in mine.values()), (rank, w, feature)
