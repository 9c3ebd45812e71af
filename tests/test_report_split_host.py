"""Host logic of the synchronous report in two phases (``rings.report_issue`` -> build the Report, empty the rings ->
``rings.report_wait``; reporting._report_split_from_plan), on the CPU checker: a subclass of its rings offers the two calls
by splitting its own ``report_fused`` -- the results are computed at the issue, taken out of the block and handed back by the
wait, so whatever read the block in between would read poison -- and records the order of what the generator does."""
import types
import weakref

import numpy as np
import pytest

from nvrx_straggler import Statistic, backend
from nvrx_straggler import reporting as reporting_mod
from nvrx_straggler.reporting import ReportGenerator
from oracle_backend import OracleBackend, OracleRingsFused

S, N, RANKS = 5, 21, 3
SCORES = ["relative_perf_scores", "individual_perf_scores"]
NO_KERNELS = {}  # (one object: a plan serves the reports that hand it the same name tables)


class SplitRings(OracleRingsFused):
    """The checker's fused rings with ``report_issue`` / ``report_wait``; ``calls`` is the order of events."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.calls = []
        self.wait_raises = None  # an exception the next wait raises
        self.names_word = None   # what the next wait leaves in meta[0]
        self._held = None
        self.live_at_general_path = "not reached"

    def report_fused(self, *a, **k):
        self.calls.append("fused")
        return super().report_fused(*a, **k)

    def report_issue(self, ws, rows_active, stats_rows, do_indiv, do_rel, thresholds, direct=None, names_ok=True,
                     order_after=None, resident=True):
        assert self._held is None, "a second issue while a report is pending"
        self.calls.append("issue")
        seq = OracleRingsFused.report_fused(self, ws, rows_active, stats_rows, do_indiv, do_rel, thresholds, direct,
                                            names_ok=names_ok, wait=True, order_after=order_after, resident=resident)
        self._held = (ws, ws._host.copy())  # "still running": nothing of this report is in the block before the wait
        ws._host[:] = 0xFF
        return seq

    def report_wait(self, ws):
        self.calls.append("wait")
        held, self._held = self._held, None
        assert held is not None and held[0] is ws, "a wait without its issue"
        if self.wait_raises is not None:
            exc, self.wait_raises = self.wait_raises, None
            ws._live = None  # (what the product's binding does when its wait fails)
            raise exc
        ws._host[:] = held[1]
        if self.names_word is not None:
            ws.meta[0], self.names_word = self.names_word, None

    def reset(self):
        self.calls.append("reset")
        super().reset()

    def report_local(self, ws, names_ok, rows_active=0):
        if self._held is None and "issue" in self.calls and self.live_at_general_path == "not reached":
            ref = ws._live  # the general path right behind an abandoned planned report
            self.live_at_general_path = None if ref is None else ref()
        return super().report_local(ws, names_ok, rows_active=rows_active)


class SplitBackend(OracleBackend):
    def make_rings(self, local_ranks, rows_per_rank, ring_cap):
        return SplitRings(self, local_ranks, rows_per_rank, ring_cap)


def _window(t):
    """[RANKS * S, N] samples of window ``t``: rank 1 is slow in section 2, more so in later windows."""
    base = np.linspace(1.0, 2.0, N, dtype=np.float32)
    out = np.empty((RANKS * S, N), dtype=np.float32)
    for lr in range(RANKS):
        for s in range(S):
            slow = np.float32(1.6 + 0.1 * t) if (lr == 1 and s == 2) else np.float32(1.0)
            out[lr * S + s] = base * np.float32(1 + s) * np.float32(1.0 + 0.01 * t) * slow
    return out


def _arm(rings, t):
    rings.samples[: RANKS * S, :N] = _window(t)
    rings.total[: RANKS * S] = N


def _setup(be, **gen_kw):
    backend.set_backend(be)
    rings = be.make_rings(RANKS, S, 64)
    rows = {f"s{i}": rings.row_for(0, f"s{i}") for i in range(S)}
    gen = ReportGenerator(SCORES, gather_on_rank0=gen_kw.pop("gather_on_rank0", True), node_name="n", **gen_kw)
    return rings, rows, gen


def _read(rep):
    """Everything a caller can read of a report, materialised."""
    found = rep.identify_stragglers()

    def exact(m):  # (float.hex: equal means the same value, and a NaN -- no kernels, no GPU score -- equals a NaN)
        return {k: float(v).hex() for k, v in m.items()}

    return {
        "rel": {k: exact(v) for k, v in rep.section_relative_perf_scores.items()},
        "indiv": {k: exact(v) for k, v in rep.section_individual_perf_scores.items()},
        "gpu_rel": exact(rep.gpu_relative_perf_scores),
        "gpu_indiv": exact(rep.gpu_individual_perf_scores),
        "stats": {k: exact(v) for k, v in rep.local_section_summaries.items()},
        "found": {k: set(v) if isinstance(v, (set, frozenset)) else {n: set(r) for n, r in v.items()} for k, v in found.items()},
    }


def _play(be, windows, reset, **gen_kw):
    rings, rows, gen = _setup(be, **gen_kw)
    out = []
    for t in range(windows):
        _arm(rings, t)
        rep = gen.generate_report_from_rings(rings, rows, NO_KERNELS, local_ranks=RANKS, reset_rings=reset)
        out.append(_read(rep))
        if reset:
            assert not rings.total.any(), f"window {t}: the rings were not emptied"
    return out, rings, gen


@pytest.fixture(autouse=True)
def _restore_backend():
    before = backend._backend
    yield
    backend.set_backend(before)


@pytest.fixture
def order(monkeypatch):
    """Record ``attach`` and ``report`` (the Report's construction) into the calls of the rings under test."""
    box = types.SimpleNamespace(rings=None)
    real = reporting_mod.Report._from_device.__func__

    def from_device(cls, *a, **k):
        if box.rings is not None:
            box.rings.calls.append("report")
        return real(cls, *a, **k)

    monkeypatch.setattr(reporting_mod.Report, "_from_device", classmethod(from_device))
    return box


def test_the_report_is_built_and_the_rings_emptied_between_issue_and_wait(order):
    be = SplitBackend(emulate_fused=True)
    rings, rows, gen = _setup(be)
    order.rings = rings
    for t in range(4):
        _arm(rings, t)
        del rings.calls[:]
        rep = gen.generate_report_from_rings(rings, rows, NO_KERNELS, local_ranks=RANKS, reset_rings=True)
        if t == 0:
            # the general path (names are being learnt): no plan yet, the rings are emptied at the end
            assert "issue" not in rings.calls and rings.calls[-1] == "reset", rings.calls
        else:
            assert rings.calls == ["issue", "report", "reset", "wait"], rings.calls
        assert not rings.total.any()
        assert {x.rank for x in rep.identify_stragglers()["straggler_sections_relative"]["s2"]} == {1}
    # without reset_rings nobody empties them
    _arm(rings, 5)
    del rings.calls[:]
    gen.generate_report_from_rings(rings, rows, NO_KERNELS, local_ranks=RANKS)
    assert rings.calls == ["issue", "report", "wait"] and rings.total[: RANKS * S].all()


def test_results_equal_the_one_call_paths(monkeypatch):
    split, rings, _ = _play(SplitBackend(emulate_fused=True), 6, True)
    assert rings.calls.count("issue") == 5 and "fused" not in rings.calls
    one_call, _, _ = _play(OracleBackend(emulate_fused=True), 6, True)  # (these rings have no report_issue: today's path)
    monkeypatch.setenv("NVRX_DEBUG_REPORT_SPLIT", "0")
    switched_off, rings0, _ = _play(SplitBackend(emulate_fused=True), 6, True)
    assert "issue" not in rings0.calls and "wait" not in rings0.calls and rings0.calls.count("fused") == 5
    for t in range(6):
        assert split[t] == one_call[t], t
        assert split[t] == switched_off[t], t
        assert {x.rank for x in split[t]["found"]["straggler_sections_relative"]["s2"]} == {1}
    assert split[1] != split[2]  # (the windows differ: equal results are not one result six times)


def test_a_held_report_keeps_its_values_across_the_next_reports():
    be = SplitBackend(emulate_fused=True)
    rings, rows, gen = _setup(be)
    held = []
    for t in range(5):
        _arm(rings, t)
        held.append(gen.generate_report_from_rings(rings, rows, NO_KERNELS, local_ranks=RANKS, reset_rings=True))
    fresh, _, _ = _play(OracleBackend(emulate_fused=True), 5, True)
    for t in range(5):  # read only now: every block was reused (and poisoned by later issues) in between
        assert _read(held[t]) == fresh[t], t


def test_ids_missing_takes_the_general_path_and_leaves_no_live_reference():
    be = SplitBackend(emulate_fused=True)
    rings, rows, gen = _setup(be)
    for t in range(2):
        _arm(rings, t)
        gen.generate_report_from_rings(rings, rows, NO_KERNELS, local_ranks=RANKS)
    _arm(rings, 2)
    del rings.calls[:]
    rings.names_word = 0
    scored = be.score_calls
    rep = gen.generate_report_from_rings(rings, rows, NO_KERNELS, local_ranks=RANKS)
    assert rings.calls[:2] == ["issue", "wait"], rings.calls
    assert be.score_calls == scored + 2  # the planned report's, then the general path's own
    assert rings.live_at_general_path is None  # the abandoned Report was nobody's by then
    want, _, _ = _play(OracleBackend(emulate_fused=True), 3, False)
    assert _read(rep) == want[2]
    # and the next report is planned again
    _arm(rings, 3)
    del rings.calls[:]
    gen.generate_report_from_rings(rings, rows, NO_KERNELS, local_ranks=RANKS)
    assert rings.calls == ["issue", "wait"], rings.calls


def test_a_wait_that_raises_drops_the_plan():
    be = SplitBackend(emulate_fused=True)
    rings, rows, gen = _setup(be)
    for t in range(2):
        _arm(rings, t)
        gen.generate_report_from_rings(rings, rows, NO_KERNELS, local_ranks=RANKS, reset_rings=True)
    plan = gen._ring_plan
    assert plan is not None
    _arm(rings, 2)
    rings.wait_raises = RuntimeError("the wait gave up")
    with pytest.raises(RuntimeError, match="gave up"):
        gen.generate_report_from_rings(rings, rows, NO_KERNELS, local_ranks=RANKS, reset_rings=True)
    assert gen._ring_plan is None and plan.ws._live is None and gen._rings_were_reset is False
    # the next report starts over on the general path and is right
    _arm(rings, 3)
    del rings.calls[:]
    rep = gen.generate_report_from_rings(rings, rows, NO_KERNELS, local_ranks=RANKS, reset_rings=True)
    assert "issue" not in rings.calls and rings.calls[-1] == "reset"
    want, _, _ = _play(OracleBackend(emulate_fused=True), 4, True)
    assert _read(rep) == want[3]


def test_a_timed_out_wait_retires_the_workspace():
    """The product's binding (backend.HipRings.report_wait) on a library whose wait times out."""
    from nvrx_straggler import _native
    from nvrx_straggler.backend import HipRings

    retired = []
    rings = HipRings.__new__(HipRings)
    rings.ctx = None
    rings.backend = types.SimpleNamespace(retire_workspace=retired.append)
    block = types.SimpleNamespace(desc_ref=None, _live=weakref.ref(rings))
    ws = types.SimpleNamespace(block=block)
    rings.lib = types.SimpleNamespace(nvrx_report_wait=lambda ctx, ref: _native.ERR_TIMEOUT)
    with pytest.raises(_native.NativeError):
        rings.report_wait(ws)
    assert retired == [ws] and block._live is None
    # any other failure lets go of the block and retires nothing
    del retired[:]
    block._live = weakref.ref(rings)
    rings.lib = types.SimpleNamespace(nvrx_report_wait=lambda ctx, ref: _native.ERR_STATE)
    with pytest.raises(_native.NativeError):
        rings.report_wait(ws)
    assert retired == [] and block._live is None
    rings.lib = types.SimpleNamespace(nvrx_report_wait=lambda ctx, ref: 0)
    block._live = keep = weakref.ref(rings)
    rings.report_wait(ws)
    assert block._live is keep


def test_a_rank_that_returns_none_builds_nothing_and_waits(order, monkeypatch):
    from nvrx_straggler import dist_utils

    monkeypatch.setattr(dist_utils, "world_and_rank", lambda group=None, cache=None: (1, 1))
    monkeypatch.setattr(dist_utils, "get_rank", lambda group=None: 1)
    be = SplitBackend(emulate_fused=True)
    rings, rows, gen = _setup(be, gather_on_rank0=True)
    order.rings = rings
    for t in range(3):
        _arm(rings, t)
        del rings.calls[:]
        rep = gen.generate_report_from_rings(rings, rows, NO_KERNELS, local_ranks=RANKS, reset_rings=True)
        assert rep is None
        if t:
            assert rings.calls == ["issue", "reset", "wait"], rings.calls
        assert not rings.total.any()


def test_the_switch_keeps_the_one_call(monkeypatch):
    monkeypatch.setenv("NVRX_DEBUG_REPORT_SPLIT", "0")
    _, rings, gen = _play(SplitBackend(emulate_fused=True), 4, True)
    assert gen._report_split is False
    assert "issue" not in rings.calls and "wait" not in rings.calls
    # one call, then the reset at the end
    assert rings.calls[-2:] == ["fused", "reset"], rings.calls
