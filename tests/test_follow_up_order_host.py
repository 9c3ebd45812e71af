"""The order of what follows a report (``ReportGenerator._follow_ups``, then ``_ring_steps``), on a box without a GPU: the job
of tests/full_report_script.py with every option on, on the composed checker, whose step entries -- the backend's and the
rings' -- are wrapped here so that each call made by the generator appends its name to a list.  Every route issues the same
steps in the same order; only the entries differ (``rings.report_<x>`` on the one-call routes, ``backend.<x>`` on the
others).  Also: what a rank without a report issues, what a generator without options issues, when rings that lack an entry
are refused, and which reporters ``straggler._Lane.build`` declines."""
import types

import pytest

import full_report_script as fs
from full_oracle_backend import FullOracleBackend

# ---- the contract, written out: step by step, in the order every route issues them ---------------------------------------------
TABLE_STEPS = ["attribution", "robust", "work", "peer", "peer_history", "peer_trend", "pace_group", "node", "history", "trend"]
RING_LOCALS = ["tail_local", "onset_local", "period_local", "episode_local", "slack_local"]
RING_STEPS = ["tail_local", "tail_group", "onset_local", "onset_group", "period_local", "period_group",
              "episode_local", "episode_group", "slack_local", "slack_group"]

# step -> its entry: on the backend (stepwise, given ws.table), on the rings (one call)
STEPWISE = {"attribution": "attribute", "robust": "robust_score", "work": "work_groups", "peer": "peer_score",
            "peer_history": "peer_history", "peer_trend": "peer_trend", "pace": "pace_score", "pace_group": "pace_group_score",
            "node": "node_score", "history": "score_history", "trend": "score_trend"}
ONE_CALL = {"attribution": "report_attribute", "robust": "report_robust", "work": "report_work", "peer": "report_peer",
            "peer_history": "report_peer_history", "peer_trend": "report_peer_trend", "pace": "report_pace",
            "pace_group": "report_pace_group", "node": "report_node", "history": "report_history", "trend": "report_trend"}
# the ring steps have one form: the local kernel on the rings, the score on the backend
RING_ENTRIES = {**{name: ("rings", name) for name in RING_LOCALS},
                **{f"{f}_group": ("backend", f"{f}_group_score") for f in ("tail", "onset", "period", "episode", "slack")},
                **{f"{f}_plain": ("backend", f"{f}_score") for f in ("tail", "onset", "period", "episode", "slack")}}
# the report itself, ahead of them
HEAD = {"general": ["report_local", "score"], "stepwise": ["report_local", "score"], "one_call": ["report_fused"],
        "one_call_async": ["report_fused"], "split": ["report_issue", "report_wait"]}
ROUTES = list(HEAD)[1:]  # (the general path is every job's first report)


class _SplitMixin:
    """``report_issue`` / ``report_wait`` for the checker's fused rings, as tests/test_report_split_host.py::SplitRings (the
    checker computes at the issue)."""

    def report_issue(self, ws, rows_active, stats_rows, do_indiv, do_rel, thresholds, direct=None, names_ok=True,
                     order_after=None, resident=True):
        return self.report_fused(ws, rows_active, stats_rows, do_indiv, do_rel, thresholds, direct, names_ok=names_ok,
                                 wait=True, order_after=order_after, resident=resident)

    def report_wait(self, ws):
        pass


class _Recorder:
    """Wraps the entries of one backend and its rings: ``calls`` is ``[(owner, entry name)]`` of the calls the generator
    made.  A call made from inside another wrapped call (the checker's ``report_attribute`` goes through its backend's
    ``attribute``) is the checker's own business and is left out."""

    BACKEND = sorted(set(STEPWISE.values()) | {e for o, e in RING_ENTRIES.values() if o == "backend"} | {"score"})
    RINGS = sorted(set(ONE_CALL.values()) | set(RING_LOCALS) | {"report_local", "report_fused", "report_issue", "report_wait"})

    def __init__(self):
        self.calls, self._depth = [], 0

    def wrap(self, obj, owner, names):
        for name in names:
            if hasattr(obj, name):
                setattr(obj, name, self._wrapped(owner, name, getattr(obj, name)))

    def _wrapped(self, owner, name, fn):
        def call(*a, **kw):
            if not self._depth:
                self.calls.append((owner, name))
            self._depth += 1
            try:
                return fn(*a, **kw)
            finally:
                self._depth -= 1

        return call


def _expected(route, table=TABLE_STEPS, ring=RING_STEPS):
    one_call = route in ("one_call", "one_call_async", "split")
    return ([("rings", e) if e.startswith("report_") else ("backend", e) for e in HEAD[route]]
            + [("rings", ONE_CALL[s]) if one_call else ("backend", STEPWISE[s]) for s in table]
            + [RING_ENTRIES[s] for s in ring])


class _Run:
    """One job of tests/full_report_script.py on a recorded checker of its own.  ``lacking``: a ``report_<x>`` these rings
    do not have."""

    def __init__(self, route, features=None, lacking=None, **options):
        from nvrx_straggler import backend

        self.route, self.rec = route, _Recorder()
        be = self.be = FullOracleBackend(emulate_fused=route != "stepwise")
        backend.set_backend(be)
        self.job = fs.Job(be, features, asynchronous=route == "one_call_async", **options)
        rings = self.job.rings
        extra = {}
        if lacking is not None:
            def missing(self):
                raise AttributeError(lacking)

            extra[lacking] = property(missing)
        if route == "split" or extra:
            bases = ((_SplitMixin,) if route == "split" else ()) + (type(rings),)
            rings.__class__ = type("RecordedRings", bases, extra)
        self.rec.wrap(be, "backend", _Recorder.BACKEND)
        self.rec.wrap(rings, "rings", _Recorder.RINGS)

    def report(self, window):
        """The calls of one report, and the report."""
        del self.rec.calls[:]
        rep = self.job.report(window)
        return list(self.rec.calls), rep

    def close(self):
        from nvrx_straggler import backend

        self.job.close()
        backend.set_backend(None)


@pytest.fixture
def run():
    made = []

    def make(*a, **kw):
        made.append(_Run(*a, **kw))
        return made[-1]

    yield make
    for r in made:
        r.close()


# ---- 1. every route, the one order ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", ["labels", "auto"])
@pytest.mark.parametrize("route", ROUTES)
def test_every_route_issues_the_steps_in_the_one_order(run, route, spec):
    r = run(route, **({} if spec == "labels" else {"peer_groups": "auto"}))
    calls, rep = r.report(0)
    assert calls == _expected("general") and rep is not None  # names are being learnt: the general path
    for w in (1, 2):
        calls, rep = r.report(w)
        assert calls == _expected(route), (route, w)
        assert rep is not None and (route != "split" or rep.generate_report_elapsed_time > 0.0)
    assert r.job.gen._last_plan_fused is (route != "stepwise")


def test_the_literal_is_the_documented_order():
    """attribution, robust, work, peer, peer history, peer trend, pace (per group here), node, history, trend; then the row
    families in ``row_families.FAMILIES`` order, then slack."""
    from nvrx_straggler import row_families

    assert TABLE_STEPS == ["attribution", "robust", "work", "peer", "peer_history", "peer_trend", "pace_group", "node",
                           "history", "trend"]
    assert RING_LOCALS == [f.name + "_local" for f in row_families.FAMILIES] + ["slack_local"]
    assert RING_STEPS[0::2] == RING_LOCALS and RING_STEPS[1::2] == [n[:-6] + "_group" for n in RING_LOCALS]


def test_job_wide_pace_and_plain_ring_scores_take_the_same_places(run):
    """Without the per-peer-group variants the pace step and the ring steps' scores are the job-wide entries, where the
    grouped ones were."""
    features = [f for f in fs.FEATURES]
    options = {"pace_peer_groups": False, "row_peer_groups": False, "slack_peer_groups": False}
    table = [s if s != "pace_group" else "pace" for s in TABLE_STEPS]
    ring = [s.replace("_group", "_plain") for s in RING_STEPS]
    for route in ("stepwise", "one_call"):
        r = run(route, features, **options)
        assert r.report(0)[0] == _expected("general", table, ring)
        assert r.report(1)[0] == _expected(route, table, ring)


# ---- 2. a rank that holds no report --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_a_rank_without_a_report_issues_no_table_follow_up_and_every_ring_step(run, route, monkeypatch):
    from nvrx_straggler import dist_utils

    monkeypatch.setattr(dist_utils, "world_and_rank", lambda group=None, cache=None: (1, 1))
    monkeypatch.setattr(dist_utils, "get_rank", lambda group=None: 1)
    r = run(route)  # (gather_on_rank0=True: rank 1 of a gathering generator)
    for w, path in ((0, "general"), (1, route), (2, route)):
        calls, rep = r.report(w)
        assert rep is None
        assert calls == _expected(path, table=[], ring=RING_LOCALS), (route, w, calls)


# ---- 3. no options, no follow-up call ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_a_generator_without_options_makes_no_follow_up_call(run, route):
    r = run(route, ["scores"])
    gen = r.job.gen
    assert gen._table_steps_on is False and gen._ring_steps_on is False and gen._one_call_needs == ()
    for w, path in ((0, "general"), (1, route), (2, route)):
        calls, rep = r.report(w)
        assert calls == _expected(path, table=[], ring=[]) and rep is not None, (route, w, calls)


# ---- 4. rings that lack an entry are refused before anything is issued -------------------------------------------------------
LACKING = [("kernel_attribution=2", "report_attribute", {}), ("robust_scores", "report_robust", {}),
           ("work_groups", "report_work", {}), ("peer_groups", "report_peer", {}),
           ("pace_scores", "report_pace", {"pace_peer_groups": False}), ("pace_peer_groups", "report_pace_group", {}),
           ("node_scores", "report_node", {}), ("peer_history", "report_peer_history", {}),
           ("peer_trends", "report_peer_trend", {}), ("score_history", "report_history", {}),
           ("score_trends", "report_trend", {})]


@pytest.mark.parametrize("option,method,options", LACKING, ids=[m for _, m, _ in LACKING])
def test_rings_without_an_entry_are_refused_before_any_call(run, option, method, options):
    r = run("one_call", lacking=method, **options)
    assert not hasattr(r.job.rings, method)
    assert r.report(0)[0][:2] == _expected("general")[:2]  # (the general path asks nothing of the rings' one-call entries)
    with pytest.raises(RuntimeError) as err:
        r.report(1)
    assert str(err.value) == f"{option}: these rings run the one-call report but have no {method}"
    assert r.rec.calls == [] and r.job.gen._ring_plan is None  # nothing was issued, and the caller dropped the plan


def test_the_refusal_checks_each_option_that_is_on_and_no_other(run):
    gen = run("one_call").job.gen
    assert gen._one_call_needs == (("kernel_attribution=2", "report_attribute"), ("robust_scores", "report_robust"),
                                   ("work_groups", "report_work"), ("peer_groups", "report_peer"),
                                   ("pace_peer_groups", "report_pace_group"), ("node_scores", "report_node"),
                                   ("peer_history", "report_peer_history"), ("peer_trends", "report_peer_trend"),
                                   ("score_history", "report_history"), ("score_trends", "report_trend"))
    assert run("one_call", ["node"]).job.gen._one_call_needs == (("node_scores", "report_node"),)


# ---- 5. the lane declines: each option alone ---------------------------------------------------------------------------------
ALONE = [{"kernel_attribution": 2}, {"tail_q_ppm": 900000}, {"onset_seg_ppm": 50000}, {"period_max": 1024},
         {"episode_len_ppm": 5000}, {"robust_scores": True}, {"peer_groups": (0, 0, 1, 1)}, {"peer_groups": ("block", 4)},
         {"work_groups": True}, {"pace_scores": True}, {"node_scores": True}, {"score_history": 8}, {"collective_slack": True}]


def _lane_det(**options):
    """What ``_Lane.build`` is handed, as the per-feature tests build it: a reporter that carries the option under test and
    little else."""

    class Reached(Exception):
        pass

    class Manager:
        is_initialized = True

        @property
        def cupti_ext(self):
            raise Reached  # what _Lane.build asks for right after its option checks

    reporter = types.SimpleNamespace(**{"_ring_plan": types.SimpleNamespace(fused=True, ws=None), "world_size": 1,
                                        "_exchanged": lambda: True, "_direct": None, "asynchronous": False,
                                        "kernel_attribution": 0, **options})
    rings = types.SimpleNamespace(lib=types.SimpleNamespace(nvrx_window_report=object()))
    return types.SimpleNamespace(_rings=rings, reporter=reporter, _cupti_manager=Manager(), _pending_region_switch=None), Reached


@pytest.mark.parametrize("option", ALONE, ids=lambda o: next(iter(o)))
def test_the_lane_declines_each_option_alone(option):
    from nvrx_straggler import reporting, straggler

    det, reached = _lane_det()
    with pytest.raises(reached):
        straggler._Lane.build(det)  # (nothing on: the option checks are passed)
    off = {k: (None if k == "peer_groups" else type(v)()) for k, v in option.items()}
    det, reached = _lane_det(**off)
    with pytest.raises(reached):
        straggler._Lane.build(det)  # (there and off)
    det, reached = _lane_det(**option)
    assert straggler._Lane.build(det) is None
    assert any(reporting.steps_behind_report(det.reporter))


def test_the_lane_and_the_generator_ask_the_same_question(run):
    from nvrx_straggler import reporting

    for features in (["scores"], ["attribution"], ["tail"], ["slack"], ["history"], None):
        gen = run("stepwise", features).job.gen
        assert reporting.steps_behind_report(gen) == (gen._table_steps_on, gen._ring_steps_on)
        assert (gen._table_steps_on, gen._ring_steps_on) == (bool(gen._one_call_needs),
                                                              bool(gen._row_families or gen.collective_slack))
