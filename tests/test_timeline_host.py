"""Timeline scores without a GPU: the option's refusals word for word, ``NVRX_TIMELINE_SCORES`` / ``NVRX_TIMELINE_BUCKETS``,
what an off generator and an off report hold, and the C entries' argument checks through the library loaded without a device."""
import ctypes
import os

import pytest

from full_oracle_backend import FullOracleBackend
from nvrx_straggler import _native

REL = ["relative_perf_scores"]


class _Checker(FullOracleBackend):
    """The CPU checker with the name of the step it does not restate: construction only asks whether the step exists."""
    timeline_score = staticmethod(lambda *a, **k: None)


@pytest.fixture
def checker():
    from nvrx_straggler import backend

    backend.set_backend(_Checker())
    try:
        yield
    finally:
        backend.set_backend(None)


@pytest.mark.parametrize("options,message", [
    ({"timeline_buckets": 3}, "timeline_buckets must be an integer within [4, 64], got 3"),
    ({"timeline_buckets": 65}, "timeline_buckets must be an integer within [4, 64], got 65"),
    ({"timeline_buckets": 32.0}, "timeline_buckets must be an integer within [4, 64], got 32.0"),
    ({"timeline_min_rows": 0}, "timeline_min_rows must be an integer within [1, 65536], got 0"),
    ({"timeline_min_effect": 0.0}, "timeline_min_effect must be a number within (0, 1], got 0.0"),
    ({"timeline_min_effect": "x"}, "timeline_min_effect must be a number within (0, 1], got 'x'"),
    ({"timeline_min_breadth": 1.5}, "timeline_min_breadth must be a number within (0, 1], got 1.5"),
    ({"timeline_buckets": 8, "timeline_min_buckets": 9},
     "timeline_min_buckets must be an integer within [1, timeline_buckets=8], got 9"),
    ({"scores_to_compute": ["individual_perf_scores"]},
     "timeline_scores needs relative_perf_scores among scores_to_compute (got ['individual_perf_scores']): timeline scores "
     "compare ranks"),
    # behind every other option's check: a bad older option is reported first
    ({"timeline_buckets": 3, "tail_profile": (0.99, 0.9)}, "tail_profile quantiles must strictly ascend, got (0.99, 0.9)"),
])
def test_the_option_is_refused_message_by_message(checker, options, message):
    from nvrx_straggler.reporting import ReportGenerator

    options = dict(options)
    with pytest.raises(ValueError) as raised:
        ReportGenerator(options.pop("scores_to_compute", REL), node_name="n", timeline_scores=True, **options)
    assert str(raised.value) == message


@pytest.mark.parametrize("env,want", [({}, 0), ({"NVRX_TIMELINE_SCORES": "0", "NVRX_TIMELINE_BUCKETS": "x"}, 0),
                                      ({"NVRX_TIMELINE_SCORES": "1"}, 32),
                                      ({"NVRX_TIMELINE_SCORES": "1", "NVRX_TIMELINE_BUCKETS": "16"}, 16)])
def test_the_environment_and_what_an_off_generator_holds(checker, monkeypatch, env, want):
    from nvrx_straggler import Detector
    from nvrx_straggler.folded import FoldedJob
    from nvrx_straggler.reporting import steps_behind_report
    from test_slack_host import _blank_report

    for name in [n for n in os.environ if n.startswith("NVRX_")]:
        monkeypatch.delenv(name)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    job = FoldedJob(total_ranks=2, sections=1, ring_cap=16, timeline_scores=bool(want), timeline_buckets=want or 32)
    try:
        Detector.initialize(node_name="n0")  # (a bad NVRX_TIMELINE_BUCKETS is read only behind every other variable, and
        for reporter in (Detector.reporter, job.reporter):  # refused by the generator only where the option is on)
            assert reporter.timeline_b == want and steps_behind_report(reporter) == (False, bool(want))  # (a ring step: c10d)
            assert [k for k in vars(reporter) if k.startswith("timeline")] == (["timeline_b", "timeline_params"] if want else [])
            assert reporter._starts_option == ("timeline_scores" if want else None)
        if want:
            assert Detector.reporter.timeline_params == {"min_rows": 8, "min_effect": 0.03, "min_breadth": 0.9, "min_buckets": 2}
    finally:
        job.close()
        Detector.shutdown()
    monkeypatch.setenv("NVRX_TIMELINE_SCORES", "yes")
    with pytest.raises(ValueError, match="NVRX_TIMELINE_SCORES must be 0 or 1, got 'yes'"):
        Detector.initialize(node_name="n0")
    assert not Detector.initialized
    blank = _blank_report()
    assert blank.timeline_scores() == {} and blank.identify_timeline_stragglers() == {
        "straggler_gpus_relative": set(), "straggler_section_ranks_relative": set(), "runs": {"gpus": {}, "sections": {}}}


def test_the_c_entries_refuse_bad_arguments_without_a_device():
    lib = _native.load()
    p, ok = ctypes.c_void_p(64), 0

    def row(B=32, rows=1, stride=8, out=p):
        return lib.nvrx_row_timeline(p, p, None, rows, stride, B, out, None)

    def rank(B=32, ranks=1, K=3, S=2, effect=30000, planes=p, out=p):
        return lib.nvrx_timeline_rank(planes, ranks, B, K, S, effect, out, None)

    def score(B=32, R=4, first=0, n=4, min_rows=8, effect=30000, breadth=900000, blocks=p):
        return lib.nvrx_timeline_score(blocks, R, B, first, n, min_rows, effect, breadth, p, None)

    assert row(B=3) == row(B=65) == row(stride=_native.MAX_RING_CAP + 4) == _native.ERR_RANGE
    assert row(rows=-1) == row(stride=6) == row(out=None) == _native.ERR_INVALID and row(rows=0) == ok
    assert rank(B=3) == rank(B=65) == rank(K=_native.MAX_ROWS + 1) == rank(effect=10**9 + 1) == _native.ERR_RANGE
    assert rank(ranks=-1) == rank(planes=None) == rank(out=None) == _native.ERR_INVALID and rank(ranks=0) == ok
    assert score(B=3) == score(B=65) == score(first=3, n=2) == score(min_rows=0) == score(breadth=10**6 + 1) == _native.ERR_RANGE
    assert score(R=0) == score(blocks=None) == _native.ERR_INVALID
    assert lib.nvrx_timeline_local(None, None, 32, p, 3, 2, 0, None) == _native.ERR_INVALID  # (local_window's: no context)
