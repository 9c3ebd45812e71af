"""Co-movement groups without a GPU: the option's refusals word for word, ``NVRX_COMOVEMENT_GROUPS``, what an off generator and
an off report hold, and the C entries' argument checks through the library loaded without a device."""
import ctypes
import os

import pytest

from full_oracle_backend import FullOracleBackend
from nvrx_straggler import _native

REL = ["relative_perf_scores"]


class _Checker(FullOracleBackend):
    """The CPU checker with the names of the steps it does not restate: construction only asks whether they exist."""
    timeline_score = staticmethod(lambda *a, **k: None)
    comovement_score = staticmethod(lambda *a, **k: None)


@pytest.fixture
def checker():
    from nvrx_straggler import backend

    backend.set_backend(_Checker())
    try:
        yield
    finally:
        backend.set_backend(None)


@pytest.mark.parametrize("options,message", [
    ({"timeline_scores": False}, "comovement_groups needs timeline_scores; timeline_scores is not set"),
    ({"comovement_min_amplitude": 0.0}, "comovement_min_amplitude must be a number within (0, 1], got 0.0"),
    ({"comovement_min_amplitude": True}, "comovement_min_amplitude must be a number within (0, 1], got True"),
    ({"comovement_min_similarity": 1.5}, "comovement_min_similarity must be a number within (0, 1], got 1.5"),
    ({"comovement_min_similarity": "x"}, "comovement_min_similarity must be a number within (0, 1], got 'x'"),
    ({"comovement_min_ranks": 1}, "comovement_min_ranks must be an integer >= 2, got 1"),
    ({"comovement_min_ranks": 2.0}, "comovement_min_ranks must be an integer >= 2, got 2.0"),
    # behind the timeline's checks: a bad timeline option is reported first
    ({"comovement_min_ranks": 1, "timeline_buckets": 3}, "timeline_buckets must be an integer within [4, 64], got 3"),
])
def test_the_option_is_refused_message_by_message(checker, options, message):
    from nvrx_straggler.reporting import ReportGenerator

    with pytest.raises(ValueError) as raised:
        ReportGenerator(REL, node_name="n", **{"timeline_scores": True, "comovement_groups": True, **options})
    assert str(raised.value) == message


@pytest.mark.parametrize("env,on", [({}, False), ({"NVRX_COMOVEMENT_GROUPS": "0"}, False),
                                    ({"NVRX_TIMELINE_SCORES": "1", "NVRX_COMOVEMENT_GROUPS": "1"}, True)])
def test_the_environment_and_what_an_off_generator_holds(checker, monkeypatch, env, on):
    from nvrx_straggler import Detector
    from nvrx_straggler.folded import FoldedJob
    from test_slack_host import _blank_report

    for name in [n for n in os.environ if n.startswith("NVRX_")]:
        monkeypatch.delenv(name)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    job = FoldedJob(total_ranks=2, sections=1, ring_cap=16, timeline_scores=on, comovement_groups=on)
    try:
        Detector.initialize(node_name="n0")
        for reporter in (Detector.reporter, job.reporter):
            assert [k for k in vars(reporter) if k.startswith("comovement")] == (["comovement_params"] if on else [])
            assert reporter.comovement_params == ({"min_rows": 8, "min_amplitude": 0.01, "min_similarity": 0.8, "min_ranks": 2,
                                                   "min_amplitude_ppm": 10000, "min_similarity_ppm": 800000} if on else None)
    finally:
        job.close()
        Detector.shutdown()
    monkeypatch.setenv("NVRX_COMOVEMENT_GROUPS", "yes")
    with pytest.raises(ValueError, match="NVRX_COMOVEMENT_GROUPS must be 0 or 1, got 'yes'"):
        Detector.initialize(node_name="n0")
    assert not Detector.initialized
    blank = _blank_report()
    assert blank.comovement_groups() == {} and blank.identify_comoving_stragglers() == {
        "straggler_gpus_comoving": set(), "straggler_section_ranks_comoving": set(), "groups": {"gpus": {}, "sections": {}}}


def test_the_c_entries_refuse_bad_arguments_without_a_device():
    lib = _native.load()
    p, odd, cap = ctypes.c_void_p(64), ctypes.c_void_p(68), _native.WORK_MAX_RANKS

    def unit(R=4, B=32, min_rows=8, amplitude=10000, blocks=p, out=p):
        return lib.nvrx_comove_unit(blocks, R, B, min_rows, amplitude, out, None)

    def pairs(R=4, similarity=800000, x=p, out=p):
        return lib.nvrx_comove_pairs(x, R, similarity, out, None)

    def groups(R=4, B=32, min_rows=8, amplitude=10000, similarity=800000, blocks=p, out=p):
        return lib.nvrx_comove_groups(blocks, R, B, min_rows, amplitude, similarity, out, None)

    assert lib.nvrx_comove_words(0, 32) == _native.ERR_INVALID
    assert lib.nvrx_comove_words(4, 3) == lib.nvrx_comove_words(4, 65) == lib.nvrx_comove_words(cap + 1, 32) == _native.ERR_RANGE
    assert b"co-movement groups take at most 4096" in lib.nvrx_last_error()
    for R in (1, 64, 65, cap):
        assert lib.nvrx_comove_words(R, 4) == _native.comove_offsets(R)[5]
    assert unit(R=0) == unit(blocks=None) == unit(out=None) == unit(out=odd) == _native.ERR_INVALID
    assert unit(R=cap + 1) == unit(B=3) == unit(min_rows=0) == unit(amplitude=0) == unit(amplitude=10**6 + 1) == _native.ERR_RANGE
    assert pairs(R=0) == pairs(x=None) == pairs(x=odd) == pairs(out=odd) == _native.ERR_INVALID
    assert pairs(R=cap + 1) == pairs(similarity=0) == pairs(similarity=10**6 + 1) == _native.ERR_RANGE
    assert groups(R=-1) == groups(blocks=None) == groups(out=None) == _native.ERR_INVALID
    assert groups(B=65) == groups(min_rows=_native.MAX_ROWS + 1) == groups(amplitude=0) == groups(similarity=0) == _native.ERR_RANGE
