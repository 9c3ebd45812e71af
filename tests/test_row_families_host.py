"""The row-family table (nvrx_straggler/row_families.py) and the one path tail, onset, period and episode scores share, on the
CPU oracle backends: the table against the C header, every family alone against all four together, the order of the steps,
pickling, and a report that is read only after the next one was issued.  tests/row_family_script.py has the window."""
import os
import pickle
import re

import pytest

import row_family_script as script
from episode_oracle_backend import EpisodeOracleBackend

FAMILY_NAMES = ("tail", "onset", "period", "episode")
KERNELS = ("beat", "stretch")  # one section and two kernels


class RecordingBackend(EpisodeOracleBackend):
    """The oracle backend of all four families, noting every ``*_local`` and ``*_score`` call in order."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.calls = []
        for fam in FAMILY_NAMES:
            self._note(self, fam + "_score")

    def _note(self, obj, name):
        inner = getattr(obj, name)

        def noted(*a, **kw):
            self.calls.append(name)
            return inner(*a, **kw)

        setattr(obj, name, noted)

    def make_rings(self, *a, **kw):
        rings = super().make_rings(*a, **kw)
        for fam in FAMILY_NAMES:
            self._note(rings, fam + "_local")
        return rings


@pytest.fixture
def cpu_backend():
    from nvrx_straggler import backend

    be = RecordingBackend()
    backend.set_backend(be)
    try:
        yield be
    finally:
        backend.set_backend(None)


def _scores(rep):
    return {fam: getattr(rep, fam + "_scores")() for fam in FAMILY_NAMES}


def test_the_table_agrees_with_the_header_the_bindings_and_the_report():
    from nvrx_straggler import _native, row_families
    from nvrx_straggler.reporting import Report, ReportGenerator

    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "nvrx_straggler.h")).read()
    planes = {name.lower(): int(value) for name, value in re.findall(r"#define\s+NVRX_(\w+)_PLANES\s+(\d+)", header)}
    planes["tail"] = 1  # (one plane: the header has no constant for it)
    symbols = {name for name, _, _ in _native.SYMBOLS}
    assert tuple(f.name for f in row_families.FAMILIES) == FAMILY_NAMES
    options = set(ReportGenerator.__init__.__code__.co_varnames)
    for fam in row_families.FAMILIES:
        assert {fam.c_row, fam.c_score, fam.c_local} <= symbols, fam.name
        assert fam.planes == planes[fam.name], fam.name
        assert callable(getattr(Report, fam.name + "_scores")) and callable(getattr(Report, f"identify_{fam.name}_stragglers"))
        assert fam.option in options, fam.name
    assert set(planes) == set(FAMILY_NAMES)  # no family of the header is missing from the table


def test_every_family_alone_gives_what_all_four_together_give(cpu_backend):
    gen, rings, rows = script.make(cpu_backend, KERNELS)
    together = _scores(script.report(gen, rings, rows, KERNELS))
    assert cpu_backend.calls == [f"{fam}_{step}" for fam in FAMILY_NAMES for step in ("local", "score")]
    for fam, option in zip(FAMILY_NAMES, script.OPTIONS):
        assert together[fam]["section_relative"].keys() == {"step"} and together[fam]["kernel_" + fam + "s"].keys() == set(KERNELS)
        gen, rings, rows = script.make(cpu_backend, KERNELS, **{option: script.OPTIONS[option]})
        alone = _scores(script.report(gen, rings, rows, KERNELS))
        assert script.same(alone[fam], together[fam]), (fam, alone[fam], together[fam])
        assert all(alone[other] == {} for other in FAMILY_NAMES if other != fam), fam


def test_the_script_is_decisive(cpu_backend):
    """Every planted pattern is found on its row by its family, below 0.75; no family flags a row that is not meant for it."""
    gen, rings, rows = script.make(cpu_backend)
    rep = script.report(gen, rings, rows)
    for fam, scores in _scores(rep).items():
        for row in script.ROWS:
            per = scores["section_relative"][row]
            assert per[0] == 1.0, (fam, row, per)
            if script.MEANT_FOR.get(fam) == row:
                assert per[1] < 0.75, (fam, row, per)
            else:
                assert per[1] >= 0.75, (fam, row, per)
        flagged = getattr(rep, f"identify_{fam}_stragglers")()["straggler_sections_relative"]
        assert {n: {s.rank for s in ids} for n, ids in flagged.items()} == ({script.MEANT_FOR[fam]: {1}} if fam in script.MEANT_FOR else {})
    onset = rep.onset_scores()["section_onsets"]["step"][1]
    assert (onset["samples_ago"], onset["window"], onset["shift"]) == (16, 64, 2.0)  # (the wrapped ring, in time order)
    period = rep.period_scores()["section_periods"]["beat"][1]
    assert (period["period"], period["excess"]) == (4, 1.5)
    episode = rep.episode_scores()["section_episodes"]["stretch"][1]
    assert (episode["length"], episode["began_ago"], episode["open_ended"]) == (12, 34, False)


def test_a_pickled_report_returns_equal_dicts(cpu_backend):
    gen, rings, rows = script.make(cpu_backend, KERNELS)
    rep = script.report(gen, rings, rows, KERNELS)
    back = pickle.loads(pickle.dumps(rep))
    want, got = _scores(rep), _scores(back)
    for fam in FAMILY_NAMES:
        assert want[fam] and script.same(got[fam], want[fam]), fam
        assert getattr(back, f"identify_{fam}_stragglers")() == getattr(rep, f"identify_{fam}_stragglers")()
    assert back.episode_scores()["gpu_scores"] == back.episode_scores()["gpu_relative"]


def test_a_report_read_after_the_next_one_was_issued_is_still_its_own(cpu_backend):
    gen, rings, rows = script.make(cpu_backend, KERNELS)
    first = script.report(gen, rings, rows, KERNELS, window=0)
    second = script.report(gen, rings, rows, KERNELS, window=1)  # (the same workspace, the first still unread)
    gen2, rings2, rows2 = script.make(cpu_backend, KERNELS)
    for window, rep in ((0, first), (1, second)):
        fresh = _scores(script.report(gen2, rings2, rows2, KERNELS, window=window))
        held = _scores(rep)
        for fam in FAMILY_NAMES:
            assert held[fam] and script.same(held[fam], fresh[fam]), (window, fam)
    assert first.tail_scores()["kernel_tails"]["beat"][0] == 1000.0 and second.tail_scores()["kernel_tails"]["beat"][0] == 2000.0
