"""The tail profile without a GPU: the option's refusals, ``NVRX_TAIL_PROFILE``, what ``Detector`` and ``FoldedJob`` hand on,
the C entries' argument checks through the library loaded without a device, and the header."""
import ctypes
import os
import re

import pytest

from full_oracle_backend import FullOracleBackend
from nvrx_straggler import _native, report_options

REL = ["relative_perf_scores"]
HEADER = open(os.path.join(os.path.dirname(__file__), "..", "include", "nvrx_straggler.h")).read()


class _Checker(FullOracleBackend):
    """The CPU checker with the name of the step it does not restate: construction only asks whether the step exists."""
    profile_score = staticmethod(lambda *a, **k: None)


@pytest.fixture
def checker():
    from nvrx_straggler import backend

    backend.set_backend(_Checker())
    try:
        yield
    finally:
        backend.set_backend(None)


@pytest.mark.parametrize("options,message", [
    ({"tail_profile": (0.99, 0.9)}, "tail_profile quantiles must strictly ascend, got (0.99, 0.9)"),
    ({"tail_profile": (0.9, 0.9)}, "tail_profile quantiles must strictly ascend, got (0.9, 0.9)"),
    ({"tail_profile": (0.4, 0.9)}, "tail_profile quantiles must be within [0.5, 0.999999], got (0.4, 0.9)"),
    ({"tail_profile": (0.9, 1.0)}, "tail_profile quantiles must be within [0.5, 0.999999], got (0.9, 1.0)"),
    ({"tail_profile": (0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.99, 0.999)},
     "tail_profile takes at most 7 quantiles, got 8: (0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.99, 0.999)"),
    ({"tail_profile": 0.9}, "tail_profile must be a sequence of 1..7 strictly ascending numbers within [0.5, 0.999999] "
                            "(None or () = off), got 0.9"),
    ({"tail_profile": (0.9,), "scores_to_compute": ["individual_perf_scores"]},
     "tail_profile=(0.9,) needs relative_perf_scores among scores_to_compute (got ['individual_perf_scores']): profile scores "
     "are relative scores"),
    # behind every other option's check: a bad older option is reported first
    ({"tail_profile": (0.99, 0.9), "stall_detection": True, "stall_min_z": -1}, "stall_min_z must be a finite number >= 0, got -1"),
])
def test_the_option_is_refused_message_by_message(checker, options, message):
    from nvrx_straggler.reporting import ReportGenerator

    options = dict(options)
    with pytest.raises(ValueError) as raised:
        ReportGenerator(options.pop("scores_to_compute", REL), node_name="n", **options)
    assert str(raised.value) == message


@pytest.mark.parametrize("text,want", [("0.9,0.99,0.999", (900000, 990000, 999000)), (" 0.5 ", (500000,)), ("", ()), (None, ())])
def test_the_environment_variable_and_the_forwarded_group(checker, monkeypatch, text, want):
    from nvrx_straggler import Detector
    from nvrx_straggler.folded import FoldedJob
    from nvrx_straggler.reporting import steps_behind_report

    for name in [n for n in os.environ if n.startswith("NVRX_")]:
        monkeypatch.delenv(name)
    if text is not None:
        monkeypatch.setenv("NVRX_TAIL_PROFILE", text)
    Detector.initialize(node_name="n0")
    try:
        assert Detector.reporter.tail_profile_ppm == want
        assert steps_behind_report(Detector.reporter) == (False, bool(want))  # (a ring step: c10d, outside the lane)
    finally:
        Detector.shutdown()
    given = tuple(q / 1e6 for q in want)
    job = FoldedJob(total_ranks=2, sections=1, ring_cap=16, tail_profile=given)  # (the argument, not the variable)
    try:
        assert job.reporter.tail_profile_ppm == want and job.reporter._row_families == ()
    finally:
        job.close()
    assert ("tail_profile" in report_options.forwarded({**_off_values(), "tail_profile": given})) == bool(want)
    monkeypatch.setenv("NVRX_TAIL_PROFILE", "0.9;0.99")
    with pytest.raises(ValueError, match="NVRX_TAIL_PROFILE must be comma-separated numbers"):
        Detector.initialize(node_name="n0")
    assert not Detector.initialized


def _off_values():
    names = set(report_options.ALWAYS) | {k for g in report_options.GROUPS for k in g.keywords}
    return dict.fromkeys(names)


def test_the_c_entries_refuse_bad_arguments_without_a_device():
    lib = _native.load()
    p = ctypes.c_void_p(64)

    def row(ppm, Q=None, rows=1, stride=8):
        return lib.nvrx_row_profile(p, p, rows, stride, _native.q_array(ppm)[0] if ppm else None, len(ppm) if Q is None else Q, p, None)

    def score(Q, R=4, first=0, n=4, table=p):
        return lib.nvrx_profile_score(p, Q, table, R, 3, 2, first, n, p, p, None)

    ok = (900000, 990000)
    assert row(ok, Q=0) == row(ok, Q=8) == row((400000,)) == row((900000, 1000000)) == _native.ERR_RANGE
    assert row((990000, 900000)) == row((900000, 900000)) == row((), Q=1) == _native.ERR_INVALID
    assert row(ok, rows=-1) == row(ok, stride=6) == _native.ERR_INVALID  # (row_op_check's)
    assert row(ok, stride=_native.MAX_RING_CAP + 4) == _native.ERR_RANGE and row(ok, rows=0) == 0
    assert score(0) == score(8) == score(3, first=3, n=2) == _native.ERR_RANGE  # (the last: plane_score's)
    assert score(3, R=0) == score(3, table=None) == _native.ERR_INVALID
    q, Q = _native.q_array(ok)
    assert lib.nvrx_profile_local(None, None, q, Q, p, 3, 2, 0, None) == _native.ERR_INVALID  # (local_window's: no context)


def test_the_header_declares_the_entries_and_no_new_planes_macro():
    for entry in ("nvrx_row_profile", "nvrx_profile_score", "nvrx_profile_local"):
        assert re.search(r"^int %s\(" % entry, HEADER, re.M) and entry in {name for name, _, _ in _native.SYMBOLS}
    assert "PROFILE" not in re.findall(r"#define\s+NVRX_(\w+)_PLANES", HEADER)
    assert re.search(r"enum \{ NVRX_PROFILE_MAX_Q = (\d+) \};", HEADER).group(1) == str(_native.PROFILE_MAX_Q)
    assert int(re.search(r"#define NVRX_PROFILE_LDS_SAMPLES (\d+)", HEADER).group(1)) == _native.PROFILE_LDS_SAMPLES
    assert _native.PROFILE_LDS_SAMPLES * 4 + 7 * 1024 * 4 + 7 * (16 + 2) * 4 <= 65536  # keys + histograms + bookkeeping in 64 KB
    assert re.search(r"#define NVRX_ABI_VERSION 2\b", HEADER)
