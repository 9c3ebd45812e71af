"""Stall scores without a GPU: option validation, the ratio's conversion, the record function, the row-step table, the header's
declarations, and a generator that holds no stall state while the option is off."""
import os
import re

import pytest

from nvrx_straggler import _native, row_families
from nvrx_straggler.reporting import Report, ReportGenerator

REL = ["relative_perf_scores"]


@pytest.mark.parametrize("options,message", [
    ({"stall_min_ratio": 1.0}, "stall_min_ratio"), ({"stall_min_ratio": 1001.0}, "stall_min_ratio"),
    ({"stall_min_ratio": "fast"}, "stall_min_ratio"), ({"stall_min_ratio": float("nan")}, "stall_min_ratio"),
    ({"stall_min_z": -0.1}, "stall_min_z"), ({"stall_min_z": float("inf")}, "stall_min_z"), ({"stall_min_z": float("nan")}, "stall_min_z"),
    ({"stall_min_z": None}, "stall_min_z"), ({"stall_min_share": 1.0}, "stall_min_share"), ({"stall_min_share": -0.01}, "stall_min_share"),
    ({"stall_min_share": float("nan")}, "stall_min_share"), ({"scores_to_compute": ["individual_perf_scores"]}, "needs relative_perf_scores"),
])
def test_options_are_validated(options, message):
    options = {"scores_to_compute": REL, **options}
    with pytest.raises(ValueError, match=message):
        ReportGenerator(options.pop("scores_to_compute"), node_name="n", stall_detection=True, **options)


def test_ratio_conversion_the_record_function_and_the_row_steps():
    assert (_native.STALL_PLANES, _native.STALL_LDS_SAMPLES, _native.STALL_MIN_SAMPLES) == (7, 12032, 8)
    for ratio, ppm in ((1.5, 1500000), (1.000001, 1000001), (1000, 1000000000), (1.0000014, 1000001), (2.4999996, 2500000)):
        assert _native.stall_ratio_ppm(ratio) == ppm
    for bad in (1.0, 1.0000004, 1000.001, -2, "x", None, float("inf")):
        with pytest.raises(ValueError, match="stall_min_ratio"):
            _native.stall_ratio_ppm(bad)
    record = row_families.STALL.record
    assert record((-1.0,) * 7, ()) is None  # absent
    assert record((1.0, 1000.0, 1000.0, 0.0, 0.0, 0.0, 600.0), ()) == {
        "excess": 1.0, "pace": 1000.0, "level": 1000.0, "share": 0.0, "events": 0, "last_samples_ago": 0, "window": 600}
    assert record((50.0, 1000.0, 50000.0, 0.047, 10.0, 123.0, 10000.0), ()) == {
        "excess": 50.0, "pace": 1000.0, "level": 50000.0, "share": 0.047, "events": 10, "last_samples_ago": 123, "window": 10000}
    assert row_families.STALL.footer((1500000, 6.0, 0.01)) == {"min_ratio": 1.5, "min_z": 6.0, "min_share": 0.01}
    assert row_families.ROW_STEPS[-2:] == (row_families.RAMP, row_families.STALL) and row_families.BY_NAME["stall"] is row_families.STALL
    assert [f.name for f in row_families.FAMILIES] == ["tail", "onset", "period", "episode"]
    assert callable(Report.stall_scores) and callable(Report.identify_stall_stragglers)


def test_header_declares_the_entries_and_the_enumerator():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "nvrx_straggler.h")).read()
    for entry in ("nvrx_row_stall", "nvrx_stall_score", "nvrx_stall_local"):
        assert re.search(r"^int %s\(" % entry, header, re.M), entry
        assert entry in {name for name, _, _ in _native.SYMBOLS}
    assert re.search(r"enum \{ NVRX_STALL_PLANES = 7 \};", header) and not re.search(r"#define\s+NVRX_STALL_PLANES", header)
    assert int(re.search(r"#define NVRX_STALL_LDS_SAMPLES (\d+)", header).group(1)) == _native.STALL_LDS_SAMPLES
    assert int(re.search(r"#define NVRX_STALL_MIN_SAMPLES (\d+)", header).group(1)) == _native.STALL_MIN_SAMPLES
    assert re.search(r"#define NVRX_ABI_VERSION 2\b", header)


def test_generator_state_on_and_off():
    off, on = ReportGenerator(REL, node_name="n"), ReportGenerator(REL, node_name="n", stall_detection=True, stall_min_ratio=2)
    try:
        assert off.stall_ratio_ppm == 0 and row_families.STALL.params(off) == () and row_families.STALL not in off._row_families
        assert not hasattr(off, "stall_min_z") and not hasattr(off, "stall_min_share")
        assert row_families.STALL.params(on) == (2000000, 6.0, 0.01) and on._row_families == (row_families.STALL,)
        assert on._starts_family is row_families.STALL
    finally:
        off.close()
        on.close()
