"""``Detector``: section timing + report orchestration, MI355X edition.

API kept from the reference (straggler.py): ``CallableId`` (:35-62), ``CustomSection`` (:66-83) and
the class-level, never-instantiated ``Detector`` with ``initialize / shutdown / detection_section /
generate_report / generate_report_if_interval_elapsed / is_interval_elapsed / wrap_callables /
restore_original_callables`` (:86-407), including its error behaviour (double initialize ->
AssertionError, use before initialize -> RuntimeError("Detector is not initialized."), instantiation
-> RuntimeError).

What changed underneath:

* a section's elapsed times are appended to a DEVICE ring (pinned staging + one scatter kernel per
  flush) instead of a Python deque, so a report never converts thousands of Python floats into a
  tensor (the reference's dominant cost, straggler.py:185);
* ``profile_cuda=True`` measures GPU time in one of two ways (``ktrace.timing_mode``): per KERNEL, by kernel name,
  through rocprofiler-sdk -- the reference's CUPTI data model, the default of multi-rank jobs, fed into the device rings
  by the tracer's own thread -- or per REGION, with two device-timestamp kernels around the section on the current stream
  (single-process default).  The ranks of a job agree on one of the two at their first collective report;
* ``generate_report`` waits only for what it needs -- the traced kernels of the window (``nvrx_ktrace_sync``) or the
  region stamps -- not ``torch.cuda.synchronize()``, then runs statistics -> all-gather -> scoring on the detector's own
  HIP stream; ``asynchronous=True`` does not even wait for that.
"""
from __future__ import annotations

import ctypes
import dataclasses
import functools
import inspect
import logging
import os
import socket
import sys
import time
from collections.abc import Callable
from contextlib import contextmanager
from typing import Any, Dict, Iterable, List, Optional, Sequence, Union

from . import _native
from . import backend as _backend_mod
from . import dist_utils as _dist_utils
from . import ktrace as _ktrace
from .cupti import CuptiManager
from .interval_tracker import ReportIntervalTracker
from .reporting import Report, ReportGenerator, _LiveBlock, _PendingBlock, _ScoreSource, steps_behind_report
from .statistics import Statistic  # noqa: F401  (re-exported for callers that poke summaries)

GPU_KEY_PREFIX = "hipevent::"  # kernel-summary key of a section's GPU-time row
_log = logging.getLogger(__name__)


@dataclasses.dataclass(frozen=True)
class CallableId:
    """Names a callable as (owner object, attribute name); ``str()`` gives its section name.

    The extra optional fields exist in the reference's dataclass and are accepted for compatibility.
    """

    obj: object
    name: str
    arg_filter_fn: Optional[Callable[[inspect.BoundArguments], bool]] = None
    extra_args_fn: Optional[Callable[[inspect.BoundArguments], dict]] = None
    ignored_args: Optional[tuple] = None

    def __str__(self) -> str:
        # naming rules of the reference (straggler.py:53-62): module name, qualified class name,
        # or the class name of an instance
        o = self.obj
        if inspect.ismodule(o):
            owner = o.__name__
        elif inspect.isclass(o):
            owner = f"{o.__module__}.{o.__name__}"
        elif hasattr(o, "__class__"):
            owner = getattr(o.__class__, "__name__", o)
        else:
            owner = getattr(o, "__name__", o)
        return f"{owner}.{self.name}"


class _ElapsedRing:
    """deque-like facade (append / extend / clear / len) over one device ring row."""

    __slots__ = ("_rings", "_row")

    def __init__(self, rings, row: int):
        self._rings = rings
        self._row = row

    def append(self, value: float) -> None:
        self._rings.push(self._row, value)

    def extend(self, values: Iterable[float]) -> None:
        self._rings.push_many(self._row, list(values) if not hasattr(values, "__len__") else values)

    def clear(self) -> None:
        self._rings.set_count(self._row, 0)

    def __len__(self) -> int:
        return self._rings.count(self._row)


class CustomSection:
    """A user-defined code section (``Detector.detection_section``).

    ``cpu_elapsed_times`` holds the wall-clock durations [ms] of profiled entries, newest
    ``max_elapseds_len`` only; here it is a view of a device ring row rather than a deque.
    ``CustomSection.max_elapseds_len`` (class attribute, default 8192 as in the reference,
    straggler.py:80) is read by ``Detector.initialize`` as the ring capacity.
    """

    max_elapseds_len: int = 8 * 1024

    __slots__ = ("name", "location", "total_entry_cnt", "row", "gpu_row", "cpu_elapsed_times")

    def __init__(self, name: str, location: str, rings=None):
        self.name = name
        self.location = location
        self.total_entry_cnt = 0
        rings = rings if rings is not None else Detector.rings
        self.row = rings.row_for(_native.KIND_SECTION, name)
        self.gpu_row: Optional[int] = None
        self.cpu_elapsed_times = _ElapsedRing(rings, self.row)


_MISS = object()  # a lane that cannot serve this report says so; the general path runs
_TRACED_DISPATCH_US = 1.0  # GPU time one traced dispatch costs (the SDK's completion signal + timestamps), see _trace_every_needed


class _Lane:
    """The steady-state report as ONE Python function around ONE C call (``nvrx_window_report``).

    ``Detector.generate_report`` is a dozen small methods of four objects -- profiler harvest, occupancy check, the
    generator's plan lookup, the one-call report, ring reset -- each cheap while the interpreter is warm.  At production
    cadence (a report per minute, a report per hundreds of steps) every one of them runs COLD after a second of training
    code: ~100 interpreter-level calls cost 150-190 us around a C call of 45 (profiles/r06a/r06c_kernels_mode_breakdown.txt).
    A lane is built after a report that took the cached plan; it holds everything that report looked up, checks with a few
    attribute reads that nothing it depends on has changed, and otherwise says ``_MISS`` BEFORE anything has happened, so the
    general path -- which stays the specification -- runs as if the lane did not exist.  The generator's name-sync and
    in-flight state is read here and written by the generator's own methods; the two marked spots of
    the asynchronous hot path do a method's writes inline, in its order."""

    trace = None

    __slots__ = ("rings", "reporter", "manager", "ext", "plan", "ws", "be", "view", "versions", "wr", "group", "wr_cache",
                 "rows_used", "desc_key", "window", "window_ref", "call", "ctx", "stream", "multi", "enqueue_only",
                 "returns_none", "stats_needed", "gather_on_rank0", "rank", "token", "asynchronous")

    @classmethod
    def build(cls, det) -> Optional["_Lane"]:
        rings, reporter, manager = det._rings, det.reporter, det._cupti_manager
        plan = reporter._ring_plan
        call = getattr(getattr(rings, "lib", None), "nvrx_window_report", None)
        if plan is None or not plan.fused or call is None or manager is None or not manager.is_initialized:
            return None
        multi = reporter.world_size > 1 and reporter._exchanged()
        if (multi and reporter._direct is None) or det._pending_region_switch is not None:
            return None  # (a host-driven exchange: the report is three calls with a collective between them)
        if reporter.asynchronous and not reporter.enqueue_only():
            return None
        if any(steps_behind_report(reporter)):
            # (a table follow-up or a ring step follows the report in the generator's paths: DESIGN.md, "The follow-ups' order")
            return None
        ext = manager.cupti_ext
        ws = plan.ws
        if ws.block.desc_key is None or not ws.send_initialised:
            return None
        self = cls()
        self.rings, self.reporter, self.manager, self.ext, self.plan, self.ws = rings, reporter, manager, ext, plan, ws
        self.be = _backend_mod.get_backend()
        self.view = plan.view
        self.versions = (reporter.name_mapper.version, reporter._private_mapper.version)
        self.group, self.wr_cache = reporter.group, reporter._wr_cache
        self.wr = _dist_utils.world_and_rank(self.group, self.wr_cache)
        self.token = det._mode_agreed
        self.rows_used = rings.rows_used
        self.desc_key = ws.block.desc_key
        self.asynchronous = reporter.asynchronous
        self.enqueue_only = bool(reporter.asynchronous)
        self.multi = multi
        self.stats_needed = plan.stats_needed
        self.gather_on_rank0, self.rank = reporter.gather_on_rank0, reporter.rank
        self.returns_none = reporter.gather_on_rank0 and reporter.rank != 0
        w = self.window = _native.WindowDesc()
        if manager.per_kernel:
            if not getattr(ext, "_counting", False):
                return None  # (dispatches are not counted: a report has to synchronise the device first -- the general path does)
            cast, klib = ctypes.cast, ext._lib
            w.kt_sync = cast(klib.nvrx_ktrace_sync, ctypes.c_void_p).value
            w.kt_hold = cast(klib.nvrx_ktrace_hold, ctypes.c_void_p).value
            w.kt_counter = cast(klib.nvrx_ktrace_counter, ctypes.c_void_p).value
            w.kt_patience_s = float(ext.sync_patience_s)
            w.kt_rows_known, w.kt_keys_without_row = int(ext._rows_known), int(ext.keys_without_row)
        else:
            w.harvest_regions = 1
        w.rows_used = self.rows_used
        w.asynchronous = 1 if self.enqueue_only else 0
        self.window_ref = ctypes.byref(w)
        self.call, self.ctx, self.stream = call, rings.ctx, self.be._stream_handle
        return self

    def run(self, det):
        """The report, or ``_MISS`` (nothing has happened), or -- names incomplete on some rank -- the general path's report."""
        t0 = time.perf_counter_ns()
        tr = _Lane.trace  # (diagnostics, tools/cadence_kernels_breakdown.py: a list that collects clock marks, normally None)
        reporter, ws, rings = self.reporter, self.ws, self.rings
        # (what else a lane is built on -- the rings, the profiler, the agreed timing mode -- only changes through Detector
        #  methods that drop the lane: initialize, shutdown, _apply_pending_mode_switch)
        if (reporter._ring_plan is not self.plan or rings._rows_used != self.rows_used or reporter._resync_pending
                or reporter.asynchronous is not self.asynchronous
                or (reporter.name_mapper.version, reporter._private_mapper.version) != self.versions
                or _dist_utils.world_and_rank(self.group, self.wr_cache) != self.wr):
            return _MISS
        if self.enqueue_only:
            pend = reporter._inflight
            if pend is not None:
                # the previous asynchronous report: usually published long ago -- one look at its completion word (what
                # ReportGenerator._settle_inflight does behind a lock, a call into the library and numpy)
                blk = pend.blk
                words = getattr(blk, "meta_words", None)
                if words is not None and pend.blob is None and words[4] == pend.seq:
                    # (the writes of ReportGenerator._settle_inflight, in its order, kept inline: this is the lane's hot path)
                    reporter._inflight = None
                    reporter._prev_async_settled = True
                    if self.multi:
                        reporter._check_exchange()
                    names_missing = words[0] != 1
                else:
                    names_missing = reporter._settle_inflight()
                if names_missing:
                    # that report's table carried an "ids missing" flag: every rank is heading for the name sync now, at the
                    # start of its general path
                    reporter._sync_names_first()
                    return _MISS
        if tr is not None:
            tr.append(("checks", time.perf_counter_ns() - t0))
        cur = ws._cur
        nxt = ws.blocks[1 - cur]
        if nxt.desc_key != self.desc_key:
            rings.configure_desc(ws, nxt, self.desc_key)  # (cold: this block has not run this shape yet)
        if nxt._live is not None:
            nxt.settle()  # (its report of two reports ago: copied out if somebody still holds it)
        ws._cur, ws.block = 1 - cur, nxt
        d = nxt.desc
        if self.enqueue_only:
            d.prev_settled = 1 if reporter._prev_async_settled else 0
        if self.multi:
            d.order_after_stream, d.order_after_enabled = self.be.current_stream_handle(), 1
        elif d.order_after_enabled:
            d.order_after_enabled = 0
        d.seq = ws.seq
        if tr is not None:
            tr.append(("settle_flip_desc", time.perf_counter_ns() - t0))
        rc = self.call(self.ctx, nxt.desc_ref, self.stream, self.window_ref)
        if tr is not None:
            tr.append(("c_call", time.perf_counter_ns() - t0))
        seq = ws.seq = d.seq
        if rc == _native.WINDOW_MISS:
            ws._cur, ws.block = cur, ws.blocks[cur]  # nothing ran on the block: it is not the current one
            return _MISS
        if rc < 0:
            reporter._drop_plan()
            if rc == _native.ERR_TIMEOUT:
                self.be.retire_workspace(ws)
            _native.check(rc)
        if self.enqueue_only:
            # (the writes of ReportGenerator._report_from_plan for a report that is only enqueued, in its order, kept inline)
            reporter._prev_async_settled = False  # until somebody has seen THIS report complete
            pend = reporter._inflight = _PendingBlock(self.be, ws, seq)
            if self.returns_none:
                return None
            return Report._from_device(_ScoreSource(self.view, pend), reporter._shared_rank_to_node(),
                                       (time.perf_counter_ns() - t0) * 1e-6, self.gather_on_rank0, self.rank)
        nxt.mark_live(seq)  # (the statistics rows land under a completion word of their own: the block's next user waits for it)
        if self.multi:
            reporter._check_exchange()
        if rc == _native.WINDOW_NAMES:
            # some rank met a new name during this report's exchange: the rings still hold the window -- sync names, report again
            reporter._sync_names_first()
            return det._report_and_reset(rings, reporter)
        if self.returns_none:
            return None
        live = _LiveBlock(self.be, ws, seq, self.stats_needed)
        nxt.attach(live)
        if tr is not None:
            tr.append(("live_block", time.perf_counter_ns() - t0))
        rep = Report._from_device(_ScoreSource(self.view, live), reporter._shared_rank_to_node(),
                                  (time.perf_counter_ns() - t0) * 1e-6, self.gather_on_rank0, self.rank)
        if tr is not None:
            tr.append(("report_object", time.perf_counter_ns() - t0))
        return rep


def _peer_groups_from_env(value: str, name: str = "NVRX_PEER_GROUPS"):
    """``NVRX_PEER_GROUPS`` (and ``NVRX_NODE_GROUPS``, by ``name``): ``auto`` (peer groups only), ``block:N``, ``mod:N`` or a comma-separated list of
    integer labels, one per logical rank; unset or empty: None (off; for the nodes: ``rank_to_node``)."""
    value = value.strip()
    if not value:
        return None
    if ":" in value or value == "auto":
        return value  # (ReportGenerator checks the rule, and says that only peer groups are inferred)
    try:
        return [int(x) for x in value.split(",")]
    except ValueError:
        raise ValueError(f"{name} must be 'block:N', 'mod:N' or a comma-separated list of integers, "
                         f"got {value!r}") from None


class _DeviceSideOnDemand(type):
    """``Detector.rings`` and ``Detector.cupti_manager`` -- everything that lives on a GPU -- come into being the first
    time they are touched, on the device that is current THEN.  The reference's own example initialises the detector
    before it selects its GPU (examples/straggler/example.py:60-66: ``Detector.initialize()``, then
    ``init_process_group``, then ``torch.cuda.set_device(local_rank)``); CUPTI does not care, device memory does: rings
    created inside ``initialize`` would sit on GPU 0 in every rank of such a script."""

    @property
    def rings(cls):
        if cls._rings is None and cls.initialized:
            cls._create_device_side()
        return cls._rings

    @rings.setter
    def rings(cls, value):
        cls._rings = value

    @property
    def cupti_manager(cls):
        if cls._cupti_manager is None and cls.initialized:
            cls._create_device_side()
        return cls._cupti_manager

    @cupti_manager.setter
    def cupti_manager(cls, value):
        cls._cupti_manager = value


class Detector(metaclass=_DeviceSideOnDemand):
    """Straggler detector; class-level singleton, not meant to be instantiated.

    Class attributes after ``initialize``: ``scores_to_compute``, ``gather_on_rank0``,
    ``profiling_interval``, ``custom_sections`` (name -> CustomSection), ``cupti_manager``,
    ``reporter`` (ReportGenerator), ``report_interval_tracker``, ``original_callables``, and ``rings``
    (the device ring buffers).
    """

    # configuration (set by initialize)
    initialized: bool = False
    scores_to_compute: Sequence[str]
    gather_on_rank0: bool
    profiling_interval: int
    report_time_interval: float
    # state (``rings``: device ring buffers, one row per section / GPU-timed region; ``cupti_manager``: the profiler that
    # feeds the GPU-time rows -- both created on first use, see _DeviceSideOnDemand)
    _rings: Any = None
    _cupti_manager: Optional[CuptiManager] = None
    _device_side_args: Any = None
    custom_sections: Dict[str, CustomSection]
    original_callables: Optional[Dict[CallableId, Any]]
    # collaborators
    reporter: ReportGenerator
    report_interval_tracker: ReportIntervalTracker
    # the name -> row tables of the rows that held samples at the last report (and the rings they were derived from)
    _occupied_key: Any = None
    _active_sections: Dict[str, int] = {}
    _active_kernels: Dict[str, int] = {}
    # the GPU-timing mode has been compared across the ranks of this process group (a token of the group, or None)
    _mode_agreed: Any = None
    # the job's common mode is region timing but this rank could not switch yet (a region was open): the reason, else None
    _pending_region_switch: Optional[str] = None
    _pending_switch_said: bool = False
    # per-kernel tracing budget (kernel_trace_budget_pct, see initialize and _calibration_mark): kernels are traced on every
    # (profiling_interval x _trace_every)-th entry of a profile_cuda section; while the cost is being measured _trace_gate
    # switches tracing on and off iteration by iteration
    kernel_trace_budget_pct: float = 0.0
    kernel_trace_cost_pct: Optional[float] = None   # what the calibration estimated (None: not measured)
    kernel_trace_dispatches: Optional[int] = None    # ... and how many dispatches a traced iteration had
    _trace_every: int = 1
    _trace_gate: bool = True
    _trace_sparse: bool = False                      # fast check in detection_section: gate closed or _trace_every > 1
    _calib: Any = None                               # (marks, flags) while measuring, else None
    # the steady-state report as one function around one C call (_Lane), built after a report that took the cached plan
    _lane: Optional[_Lane] = None
    _lanes_enabled: bool = True

    def __new__(cls):
        raise RuntimeError(f"class {cls.__name__} should not be instantiated")

    # ---- lifecycle -----------------------------------------------------------------------------
    @classmethod
    def initialize(
        cls,
        scores_to_compute: Union[Sequence[str], str] = "all",
        gather_on_rank0: bool = True,
        profiling_interval: int = 1,
        report_time_interval: float = 60,
        node_name: Optional[str] = None,
        max_rows: int = 256,
        asynchronous: Optional[bool] = None,
        kernel_trace_budget_pct: Optional[float] = None,
        kernel_attribution: Optional[int] = None,
        tail_quantile: Optional[float] = None,
        robust_scores: Optional[bool] = None,
        onset_detection: Optional[bool] = None,
        onset_min_segment: float = 0.05,
        onset_min_strength: float = 0.5,
        period_detection: Optional[bool] = None,
        period_max: int = 1024,
        period_min_strength: float = 0.5,
        episode_detection: Optional[bool] = None,
        episode_min_length: float = 0.005,
        episode_min_strength: float = 0.5,
        score_history: Optional[int] = None,
        persistence_min_reports: Optional[int] = None,
        persistence_thresholds: Optional[Sequence[float]] = None,
        score_trends: Optional[bool] = None,
        trend_min_reports: Optional[int] = None,
        trend_min_tau: float = 0.6,
        trend_horizon: Optional[int] = None,
        collective_slack: Optional[bool] = None,
        slack_min_ranks: int = 4,
        slack_min_share: float = 0.05,
        slack_max_ratio: float = 0.25,
        peer_groups=None,
        peer_min_ranks: Optional[int] = None,
        peer_history: Optional[int] = None,
        peer_persistence_min_reports: Optional[int] = None,
        peer_persistence_thresholds: Optional[Sequence[float]] = None,
        peer_trends: Optional[bool] = None,
        pace_scores: Optional[bool] = None,
        pace_min_ranks: int = 4,
        pace_min_columns: int = 8,
        pace_min_effect: float = 0.03,
        pace_min_breadth: float = 0.9,
        pace_peer_groups: Optional[bool] = None,
        slack_peer_groups: Optional[bool] = None,
        row_peer_groups: Optional[bool] = None,
        node_scores: Optional[bool] = None,
        node_groups=None,
        node_min_members: int = 2,
        node_min_nodes: int = 3,
        node_min_columns: int = 8,
        node_min_effect: float = 0.03,
        node_min_breadth: float = 0.9,
        node_min_agree: float = 0.75,
        work_groups: Optional[bool] = None,
        work_count_tol: Optional[float] = None,
        work_max_unlike: Optional[float] = None,
    ):
        """
        Args:
            scores_to_compute: list with 'relative_perf_scores' and/or 'individual_perf_scores', or "all".
            gather_on_rank0: rank 0's report covers all ranks (others get None); else per-rank reports.
            profiling_interval: profile every N-th entry of a section.
            report_time_interval: seconds between reports for ``generate_report_if_interval_elapsed``.
            node_name: name of this node in reports (default: ``socket.gethostname()``).
            max_rows: timing rows (sections + GPU-timed regions) the device rings can hold.
            asynchronous: ``generate_report`` only enqueues the report on the detector's HIP stream and returns a
                ``Report`` that waits for the device when it is first read, so the training loop never stalls on a
                report (see ``ReportGenerator``).  Default: the ``NVRX_ASYNC_REPORT`` environment variable, else
                False = the reference's synchronous behaviour.
            kernel_trace_budget_pct: per-kernel tracing only (``ktrace.timing_mode() == "kernels"``).  The share of a training
                iteration that tracing every kernel of the profiled sections may cost.  rocprofiler-sdk adds about a
                microsecond to every traced dispatch, which on a step of hundreds of small kernels is more than the
                reference's "< 1 %" (docs/source/straggler_det/usage_guide.rst:169).  With a budget, the first 16 iterations
                seen by ``generate_report_if_interval_elapsed`` -- the ones the interval tracker times anyway
                (interval_tracker.py:35,58-72) -- alternate between tracing and not tracing; if the traced ones are slower
                by more than the budget, kernels are traced on every (profiling_interval x N)-th entry only, N the smallest
                multiple that fits, the LARGEST N over the ranks (one all-reduce), logged once.  Section wall times are
                still recorded at ``profiling_interval``.  Default: ``NVRX_KTRACE_BUDGET_PCT``, else 1.0; 0 = trace at
                ``profiling_interval`` whatever it costs (the reference's behaviour).  Jobs that call ``generate_report``
                themselves never calibrate.
            kernel_attribution: 0 = off; N in 1..16: every report also carries, per rank and GPU score, the N kernels with the
                largest share of the score's deficit (``Report.explain_gpu_scores()``).  Default: ``NVRX_KERNEL_ATTRIBUTION``,
                else 0.  Pass the same value on every rank (no collective depends on it).
            tail_quantile: 0 = off; q in [0.5, 0.999999]: every report also carries the q-quantile of every section and kernel
                row and relative scores built from them (``Report.tail_scores()``, ``Report.identify_tail_stragglers()``):
                they show a rank that is slow on some iterations only, which median-based scores cannot.  Needs
                ``relative_perf_scores``.  Default: ``NVRX_TAIL_QUANTILE``, else 0.  Pass the same value on EVERY rank (the
                step adds one collective per report).
            robust_scores: every report also rates each rank against the job's MEDIAN and spread instead of its fastest rank
                (``Report.robust_scores()``, ``Report.identify_robust_stragglers()``): one anomalously fast rank no longer
                flags everybody else, and the cut-off follows the job's own scatter.  Needs ``relative_perf_scores``.
                Default: ``NVRX_ROBUST_SCORES``, else off.  Pass the same value on every rank (no collective depends on it).
            onset_detection: every report also says SINCE WHEN a rank is slow: per section and kernel row the single step in
                the window's samples, in time order, that explains most of their variance, and relative scores built from the
                shifts (``Report.onset_scores()``, ``Report.identify_onset_stragglers()``).  A rank that became 1.5 x slower
                70 % of the way through a window leaves the median where it was; here it shows with the number of samples
                since the change.  Needs ``relative_perf_scores``.  Default: ``NVRX_ONSET_DETECTION``, else off.  Pass the
                same values on EVERY rank (the step adds one collective per report).
            onset_min_segment: the shortest stretch either side of a step, as a share of the row's samples, within
                [0.000001, 0.5]; never fewer than 8 samples.
            onset_min_strength: a step counts as a shift when it explains at least this share of the row's variance, within
                [0, 1].  0.5 is a default, not a measurement.
            period_detection: every report also says whether a rank is slow ON A BEAT: per section and kernel row the period,
                counted in samples of that row, on which the row stalls, the samples since the slow phase last occurred, and
                relative scores built from the excess of the slow phase over the rest (``Report.period_scores()``,
                ``Report.identify_period_stragglers()``).  A rank that is 1.5 x slower on every 50th sample moves neither its
                median nor its 0.95-quantile; here it shows as "every 50 samples, last seen 36 samples ago".  Needs
                ``relative_perf_scores``.  Default: ``NVRX_PERIOD_DETECTION``, else off.  Pass the same values on EVERY rank
                (the step adds one collective per report).
            period_max: the largest period looked for, an integer within [2, 4096]; never more than a quarter of a row's
                samples (fewer than four repetitions are not a beat).
            period_min_strength: a beat counts when its phase means explain (adjusted R^2) at least this share of the row's
                variance, within [0, 1].  0.5 is a default, not a measurement.
            episode_detection: every report also says whether a rank was slow FOR ONE STRETCH of the window and then recovered
                (a thermal excursion, a neighbour's checkpoint, a link that flapped): per section and kernel row the interval
                of its samples, in time order, that spent most time above the row's mean, how long it lasted, how many samples
                ago it ended, the means inside and outside, and relative scores built from their ratio
                (``Report.episode_scores()``, ``Report.identify_episode_stragglers()``).  A rank that is 1.5 x slower on 300
                consecutive samples of 10 000 moves neither its median nor its 0.95-quantile, and has no step and no beat;
                here it scores 0.67.  Needs ``relative_perf_scores``.  Default: ``NVRX_EPISODE_DETECTION``, else off.  Pass
                the same values on EVERY rank (the step adds one collective per report).
            episode_min_length: an episode, and the stretch of "normal" either side of it, holds at least this share of the
                row's samples, within [0.000001, 0.333333]; never fewer than 8 samples.
            episode_min_strength: an episode counts when its two levels explain at least this share of the row's variance,
                within [0, 1].  0.5 is a default, not a measurement.
            score_history: 0 = off; H in 2..64: every report also appends its scores to a history of the last H reports and
                says, per rank and score, for how many reports in a row the score has been below its threshold
                (``Report.score_history()``, ``Report.identify_persistent_stragglers()``): a rank that was slow in one window
                only -- a neighbour's checkpoint, a page-cache flush -- is not flagged, one that stays slow is.  Default:
                ``NVRX_SCORE_HISTORY``, else 0.  Pass the same value on every rank (no collective depends on it).
            persistence_min_reports: the streak that makes a rank persistently slow, within [1, score_history].  Default:
                ``NVRX_PERSISTENCE_MIN_REPORTS``, else 3 (never more than ``score_history``).
            persistence_thresholds: (gpu_rel, section_rel, gpu_indiv, section_indiv) a score has to be below; default: 0.75
                each, the thresholds the reports' own flags are computed for.
            score_trends: behind the history step, every report also estimates per rank and score whether the history's scores
                are FALLING from report to report -- the Theil-Sen slope, the trend line's level and Kendall's tau
                (``Report.score_trends()``) -- and ``Report.identify_declining_stragglers()`` names the ranks that will cross
                their threshold within ``trend_horizon`` reports, before any other rule flags them.  Needs ``score_history``
                >= 4.  Default: ``NVRX_SCORE_TRENDS`` (set and not "0"), else off.
            trend_min_reports: usable reports a trend needs, within [4, score_history].  Default: 6, or ``score_history`` where
                that is less.
            trend_min_tau: a score is falling when Kendall's tau is at most minus this, within (0, 1].
            trend_horizon: reports ahead that ``identify_declining_stragglers`` looks; None = ``score_history``.  6, 0.6 and
                that horizon are defaults, not measurements.
            collective_slack: every report also says whom the job WAITS FOR in collectives (``Report.slack_scores()``,
                ``Report.identify_slack_stragglers()``): a rank whose host is slow launches late and computes at the usual
                speed, so every other score reads 1; inside the collective kernels it spends the least time of all ranks and
                the others the wait for it on top.  Per-kernel timing only (region timing has no collective rows: the result
                is empty); needs ``relative_perf_scores``; the same value on EVERY rank (one more collective per report).
                Default: ``NVRX_COLLECTIVE_SLACK`` (set and not "0"), else off.
            slack_min_ranks: ranks a collective kernel must have been seen on to be used (never more than the job has).
            slack_min_share, slack_max_ratio: the rule of ``identify_slack_stragglers``: the typical rank waits at least
                this share of its traced GPU time, and the named rank at most this fraction of the typical wait.  4, 0.05 and
                0.25 are defaults, not measurements.
            peer_groups: which ranks do the SAME WORK -- a pipeline stage, an expert group, a role: every report also rates
                each rank against the fastest rank of its own group instead of the fastest of the whole job
                (``Report.peer_scores()``, ``Report.identify_peer_stragglers()``), so that the healthy ranks of a slower
                stage are not named.  A list, tuple or ndarray of ``int`` or ``str`` labels, one per LOGICAL rank of the job,
                or ``"block:N"`` (label ``rank // N``: contiguous stages) or ``"mod:N"`` (label ``rank % N``).  Needs
                ``relative_perf_scores``.  ``"auto"``: nobody describes the layout -- the groups of every report are the work
                groups inferred from its table (``work_groups`` below, which it implies; at most 4096 logical ranks).  Default:
                ``NVRX_PEER_GROUPS`` (``auto``, ``block:N``, ``mod:N`` or a comma-separated list of integers), else off.  Same
                value on every rank (no collective depends on it).
            peer_min_ranks: ranks of a group that must have a section or kernel for the group to have a reference; at the
                default of 2 (``NVRX_PEER_MIN_RANKS``) a rank alone in its group has no peer and is unrated, not rated 1.0.
            peer_history: 0 = off; H in 2..64: ``score_history`` for the PEER scores -- every report also appends its peer scores
                to a history of the last H reports (``Report.peer_history()``,
                ``Report.identify_persistent_peer_stragglers()``).  In a job with peer groups the job-wide history names every
                healthy rank of a slower stage; this one names the rank that stays slower than its peers.  Needs
                ``peer_groups``.  A rank unrated in a report (alone in its group) has no entry for it, which ends its streak;
                the history is per rank and does not notice that a rank's peers changed between reports
                (``peer_groups="auto"``).  Default: ``NVRX_PEER_HISTORY``, else 0.
            peer_persistence_min_reports: the streak that makes a rank persistently slower than its peers, within
                [1, peer_history].  Default: ``NVRX_PEER_PERSISTENCE_MIN_REPORTS``, else 3 (never more than ``peer_history``).
            peer_persistence_thresholds: (gpu, section) a peer score has to be strictly below; default 0.75 each, as
                ``identify_peer_stragglers``.
            peer_trends: ``score_trends`` for the peer scores (``Report.peer_trends()``,
                ``Report.identify_declining_peer_stragglers()``), by ``trend_min_reports``, ``trend_min_tau`` and
                ``trend_horizon`` (None = ``peer_history``).  Needs ``peer_history`` >= 4.  Default: ``NVRX_PEER_TRENDS`` (set
                and not "0"), else off.
            pace_scores: every report also says whether a rank is a LITTLE slower in nearly ALL of its kernels -- a card held a
                clock step down, a throttling HBM stack, a marginal power rail: 3-5 % on every kernel, which no threshold on
                one row sees (``Report.pace_scores()``, ``Report.identify_pace_stragglers()``).  Needs
                ``relative_perf_scores``.  Default: ``NVRX_PACE_SCORES`` (set and not "0"), else off.  Same value on every
                rank (no collective depends on it).
            pace_min_ranks: ranks that must have a kernel or section for its median to be a reference (clamped to the job's
                ranks).
            pace_min_columns, pace_min_effect, pace_min_breadth: the rule of ``identify_pace_stragglers``: at least this many
                columns, a pace of at most ``1 - pace_min_effect`` and slower than the job's median in at least this share of
                the columns.  8, 0.03 and 0.9 are defaults, not measurements.
            pace_peer_groups: the pace scores rate each rank against the lower median of its OWN peer group instead of the
                whole job's -- the right centre in a job of pipeline stages or expert groups, where the job's median names
                every healthy rank of the slower stage.  Needs ``pace_scores`` and ``peer_groups``; a group needs
                ``max(peer_min_ranks, min(pace_min_ranks, its size))`` ranks with a kernel for its median to be a reference.
                Default: ``NVRX_PACE_PEER_GROUPS`` ("1"; "0" or unset: off).  Same value on every rank (no collective depends
                on it).
            slack_peer_groups: the slack scores take a collective kernel's floor and the typical wait inside each rank's OWN
                peer group instead of the whole job -- the right reference in a job of pipeline stages, tensor-parallel or
                expert groups, where waits in collectives legitimately differ per stage and the job-wide rule names the
                healthy ranks of the stage that waits least, or nobody.  Needs ``collective_slack`` and ``peer_groups``
                (``"auto"`` is allowed); a (group, collective kernel) pair needs ``max(peer_min_ranks, min(slack_min_ranks,
                its size))`` ranks to be a reference.  A group of two names nobody; a rank alone in its group is unrated.
                Default: ``NVRX_SLACK_PEER_GROUPS`` ("1"; "0" or unset: off).  Same value on every rank.
            row_peer_groups: every row family that is on (``tail_quantile``, ``onset_detection``, ``period_detection``,
                ``episode_detection``) takes a column's reference inside each rank's OWN peer group instead of the whole job:
                tails are absolute times, so the job-wide rule names the healthy ranks of a slower pipeline stage, and a step,
                a beat or a stretch that one whole stage shares flags that stage.  Needs ``peer_groups`` (``"auto"`` is
                allowed) and at least one row family; a (group, column) pair needs ``peer_min_ranks`` ranks to be a reference,
                so a rank alone in its group is unrated.  Nothing else is exchanged.  Default: ``NVRX_ROW_PEER_GROUPS`` ("1";
                "0" or unset: off).  Same value on every rank.
            node_scores: every report also says whether a NODE is a little slower in nearly all of its kernels -- failed fans,
                a capped PSU, a throttling host CPU, the wrong power profile: all GPUs of one host lose a few per cent, the
                pace scores name every one of them, and only a score per node says that they are one incident
                (``Report.node_scores()``, ``Report.identify_node_stragglers()``).  Needs ``relative_perf_scores``.  The
                centre is the job's (a lockstep model); node scores inside pipeline stages are out of scope.  Default:
                ``NVRX_NODE_SCORES`` ("1"; "0" or unset: off).  No collective depends on it.
            node_groups: which logical ranks share a node: None -- ``rank_to_node`` as the name sync gathered it (needs
                ``gather_on_rank0=True``, which gathers it for every rank) --, or ``"block:N"``, ``"mod:N"`` or one label
                per logical rank, parsed as ``peer_groups`` is: the only way a folded run or a one-box test gets more than
                one node.  Default: ``NVRX_NODE_GROUPS`` (a rule, or comma-separated integer labels, as
                ``NVRX_PEER_GROUPS``).
            node_min_members: ranks of a node that must have a kernel for the node's median to count (clamped to its size).
            node_min_nodes: nodes that must have a median for a kernel to have a reference (clamped to the job's nodes).
            node_min_columns, node_min_effect, node_min_breadth, node_min_agree: the rule of ``identify_node_stragglers``:
                at least this many columns, a pace of at most ``1 - node_min_effect``, slower than the nodes' centre in at
                least this share of the columns, and at least this share of the node's rated ranks off pace themselves.
                8, 0.03, 0.9 and 0.75 are defaults, not measurements.
            work_groups: every report also says which ranks do the SAME WORK, inferred from the table the report gathers anyway
                (``Report.work_groups()``): which kernels and sections a rank has at all and how often each kernel ran do not
                depend on how fast the rank runs.  With explicit ``peer_groups`` the report also lists the labels that
                contradict the work (``"label_conflicts"``).  Needs ``relative_perf_scores``; at most 4096 logical ranks.
                Default: ``NVRX_WORK_GROUPS`` ("1"; "0" or unset: off).  No collective depends on it.
            work_count_tol, work_max_unlike: two ranks are alike when at most the share ``work_max_unlike`` of the columns either
                of them has differ, a kernel both have differing when its call counts are more than ``1 + work_count_tol`` apart.
                Defaults: ``NVRX_WORK_COUNT_TOL`` / ``NVRX_WORK_MAX_UNLIKE``, else 0.25 and 0.1 -- defaults, not measurements.
        """
        assert not cls.initialized
        _backend_mod.require_engine()  # no silent CPU path: a box that cannot run the engine says so here
        everything = str(scores_to_compute) == "all"
        cls.scores_to_compute = ["relative_perf_scores", "individual_perf_scores"] if everything else scores_to_compute
        cls.gather_on_rank0, cls.profiling_interval = gather_on_rank0, profiling_interval
        cls.report_time_interval = report_time_interval
        cls.custom_sections, cls.original_callables, cls._occupied_key = {}, {}, None

        # device side -- the rings every section / GPU-timed region records into and the profiler that feeds them --
        # is created on first use, on the device that is current then (_DeviceSideOnDemand)
        capacity = int(CustomSection.max_elapseds_len)
        per_kernel = _ktrace.timing_mode() == "kernels"
        if per_kernel and int(max_rows) == 256:
            max_rows = 4096  # one row per distinct kernel key; 4096 x 8192 f32 = 128 MB of 288 GB
        cls._rings = cls._cupti_manager = cls._lane = None
        cls._device_side_args = (int(max_rows), capacity)
        cls._mode_agreed = None
        cls._pending_region_switch, cls._pending_switch_said = None, False
        if kernel_trace_budget_pct is None:
            try:
                kernel_trace_budget_pct = float(os.environ.get("NVRX_KTRACE_BUDGET_PCT", "1.0"))
            except ValueError:
                kernel_trace_budget_pct = 1.0
        cls.kernel_trace_budget_pct = max(0.0, float(kernel_trace_budget_pct))
        cls.kernel_trace_cost_pct = None
        cls._trace_every, cls._trace_gate, cls._trace_sparse = 1, True, False
        cls._calib = ([], [], []) if (per_kernel and cls.kernel_trace_budget_pct > 0.0) else None
        cls.kernel_trace_dispatches = None
        _log.info("nvrx straggler: GPU time of profile_cuda sections is measured per %s (mode '%s': %s)",
                  "kernel, by kernel name" if per_kernel else "profiled region", _ktrace.timing_mode(), _ktrace.mode_note())

        # host side: who scores, and when
        if asynchronous is None:
            asynchronous = os.environ.get("NVRX_ASYNC_REPORT", "0") not in ("", "0")
        if kernel_attribution is None:
            try:
                kernel_attribution = int(os.environ.get("NVRX_KERNEL_ATTRIBUTION", "0") or 0)
            except ValueError:
                raise ValueError("NVRX_KERNEL_ATTRIBUTION must be an integer: 0 (off) or 1..16") from None
        if tail_quantile is None:
            tail_quantile = os.environ.get("NVRX_TAIL_QUANTILE", "") or 0.0
        if robust_scores is None:
            robust_scores = os.environ.get("NVRX_ROBUST_SCORES", "0") not in ("", "0")
        if onset_detection is None:
            onset_detection = os.environ.get("NVRX_ONSET_DETECTION", "0") not in ("", "0")
        if period_detection is None:
            period_detection = os.environ.get("NVRX_PERIOD_DETECTION", "0") not in ("", "0")
        if episode_detection is None:
            episode_detection = os.environ.get("NVRX_EPISODE_DETECTION", "0") not in ("", "0")
        if score_history is None:
            try:
                score_history = int(os.environ.get("NVRX_SCORE_HISTORY", "0") or 0)
            except ValueError:
                raise ValueError("NVRX_SCORE_HISTORY must be an integer: 0 (off) or 2..64 reports") from None
        if persistence_min_reports is None:
            from_env = os.environ.get("NVRX_PERSISTENCE_MIN_REPORTS", "")
            if from_env:
                try:
                    persistence_min_reports = int(from_env)
                except ValueError:
                    raise ValueError("NVRX_PERSISTENCE_MIN_REPORTS must be an integer within [1, NVRX_SCORE_HISTORY]") from None
            else:
                persistence_min_reports = 3
                if score_history == 2:
                    persistence_min_reports = 2  # (a history of two reports cannot hold a streak of three)
        if score_trends is None:
            score_trends = os.environ.get("NVRX_SCORE_TRENDS", "0") not in ("", "0")
        if collective_slack is None:
            collective_slack = os.environ.get("NVRX_COLLECTIVE_SLACK", "0") not in ("", "0")
        trend_min_reports_defaulted = trend_min_reports is None
        if trend_min_reports is None:
            trend_min_reports = 6
            if isinstance(score_history, int) and 4 <= score_history < 6:
                trend_min_reports = score_history  # (a history of four reports cannot hold six)
        peer_options = {}  # (off: the generator is built exactly as before)
        if peer_groups is None:
            peer_groups = _peer_groups_from_env(os.environ.get("NVRX_PEER_GROUPS", ""))
        if peer_groups is not None:
            if peer_min_ranks is None:
                try:
                    peer_min_ranks = int(os.environ.get("NVRX_PEER_MIN_RANKS", "") or 2)
                except ValueError:
                    raise ValueError("NVRX_PEER_MIN_RANKS must be an integer >= 1") from None
            peer_options = {"peer_groups": peer_groups, "peer_min_ranks": peer_min_ranks}
        if peer_history is None:
            try:
                peer_history = int(os.environ.get("NVRX_PEER_HISTORY", "0") or 0)
            except ValueError:
                raise ValueError("NVRX_PEER_HISTORY must be an integer: 0 (off) or 2..64 reports") from None
        if peer_trends is None:
            peer_trends = os.environ.get("NVRX_PEER_TRENDS", "0") not in ("", "0")
        if peer_history or peer_trends:  # (off: the generator is built exactly as before)
            if peer_persistence_min_reports is None:
                from_env = os.environ.get("NVRX_PEER_PERSISTENCE_MIN_REPORTS", "")
                if from_env:
                    try:
                        peer_persistence_min_reports = int(from_env)
                    except ValueError:
                        raise ValueError("NVRX_PEER_PERSISTENCE_MIN_REPORTS must be an integer within [1, NVRX_PEER_HISTORY]") from None
                else:
                    peer_persistence_min_reports = 2 if peer_history == 2 else 3  # (two reports cannot hold a streak of three)
            if peer_trends and trend_min_reports_defaulted and isinstance(peer_history, int) and 4 <= peer_history < trend_min_reports:
                trend_min_reports = peer_history  # (a history of four reports cannot hold six)
            peer_options.update(peer_history=peer_history, peer_persistence_min_reports=peer_persistence_min_reports,
                                peer_persistence_thresholds=peer_persistence_thresholds, peer_trends=peer_trends)
        work_options = {}  # (off: the generator is built exactly as before)
        if work_groups is None:
            from_env = os.environ.get("NVRX_WORK_GROUPS", "")
            if from_env not in ("", "0", "1"):
                raise ValueError(f"NVRX_WORK_GROUPS must be 0 or 1, got {from_env!r}")
            work_groups = from_env == "1"
        if work_groups or (isinstance(peer_groups, str) and peer_groups == "auto"):
            for name, env, default in (("work_count_tol", "NVRX_WORK_COUNT_TOL", 0.25), ("work_max_unlike", "NVRX_WORK_MAX_UNLIKE", 0.1)):
                value = work_count_tol if name == "work_count_tol" else work_max_unlike
                if value is None:
                    try:
                        value = float(os.environ.get(env, "") or default)
                    except ValueError:
                        raise ValueError(f"{env} must be a number, got {os.environ.get(env)!r}") from None
                work_options[name] = value
            if work_groups:
                work_options["work_groups"] = True
        pace_options = {}  # (off: the generator is built exactly as before)
        if pace_scores is None:
            pace_scores = os.environ.get("NVRX_PACE_SCORES", "0") not in ("", "0")
        if pace_scores:
            pace_options = {"pace_scores": True, "pace_min_ranks": pace_min_ranks, "pace_min_columns": pace_min_columns,
                            "pace_min_effect": pace_min_effect, "pace_min_breadth": pace_min_breadth}
        if pace_peer_groups is None:
            from_env = os.environ.get("NVRX_PACE_PEER_GROUPS", "")
            if from_env not in ("", "0", "1"):
                raise ValueError(f"NVRX_PACE_PEER_GROUPS must be 0 or 1, got {from_env!r}")
            pace_peer_groups = from_env == "1"
        if pace_peer_groups:
            pace_options["pace_peer_groups"] = True  # (the generator says which of pace_scores and peer_groups it misses)
        if slack_peer_groups is None:
            from_env = os.environ.get("NVRX_SLACK_PEER_GROUPS", "")
            if from_env not in ("", "0", "1"):
                raise ValueError(f"NVRX_SLACK_PEER_GROUPS must be 0 or 1, got {from_env!r}")
            slack_peer_groups = from_env == "1"
        if slack_peer_groups:
            pace_options["slack_peer_groups"] = True  # (the generator says which of collective_slack and peer_groups it misses)
        if row_peer_groups is None:
            from_env = os.environ.get("NVRX_ROW_PEER_GROUPS", "")
            if from_env not in ("", "0", "1"):
                raise ValueError(f"NVRX_ROW_PEER_GROUPS must be 0 or 1, got {from_env!r}")
            row_peer_groups = from_env == "1"
        if row_peer_groups:
            pace_options["row_peer_groups"] = True  # (the generator says which of a row family and peer_groups it misses)
        node_options = {}  # (off: the generator is built exactly as before)
        if node_scores is None:
            from_env = os.environ.get("NVRX_NODE_SCORES", "")
            if from_env not in ("", "0", "1"):
                raise ValueError(f"NVRX_NODE_SCORES must be 0 or 1, got {from_env!r}")
            node_scores = from_env == "1"
        if node_scores:
            if node_groups is None:
                node_groups = _peer_groups_from_env(os.environ.get("NVRX_NODE_GROUPS", ""), "NVRX_NODE_GROUPS")
            node_options = {"node_scores": True, "node_groups": node_groups, "node_min_members": node_min_members,
                            "node_min_nodes": node_min_nodes, "node_min_columns": node_min_columns,
                            "node_min_effect": node_min_effect, "node_min_breadth": node_min_breadth,
                            "node_min_agree": node_min_agree}
        cls.reporter = ReportGenerator(scores_to_compute=cls.scores_to_compute, gather_on_rank0=gather_on_rank0,
                                       node_name=node_name or socket.gethostname(), asynchronous=asynchronous,
                                       kernel_attribution=kernel_attribution, tail_quantile=tail_quantile,
                                       robust_scores=robust_scores, onset_detection=onset_detection,
                                       onset_min_segment=onset_min_segment, onset_min_strength=onset_min_strength,
                                       period_detection=period_detection, period_max=period_max,
                                       period_min_strength=period_min_strength, episode_detection=episode_detection,
                                       episode_min_length=episode_min_length, episode_min_strength=episode_min_strength,
                                       score_history=score_history, persistence_min_reports=persistence_min_reports,
                                       persistence_thresholds=persistence_thresholds, score_trends=score_trends,
                                       trend_min_reports=trend_min_reports, trend_min_tau=trend_min_tau,
                                       trend_horizon=trend_horizon, collective_slack=collective_slack,
                                       slack_min_ranks=slack_min_ranks, slack_min_share=slack_min_share,
                                       slack_max_ratio=slack_max_ratio, **peer_options, **pace_options, **node_options,
                                       **work_options)
        cls.report_interval_tracker = ReportIntervalTracker(time_interval=report_time_interval,
                                                            profiling_interval=profiling_interval)
        cls.report_interval_tracker.also_max = cls._trace_every_needed  # (the tracing budget's number rides on the tracker's all-reduce)
        cls.initialized = True

    @classmethod
    def _create_device_side(cls) -> None:
        if cls._rings is not None:
            return
        max_rows, capacity = cls._device_side_args
        rings = _backend_mod.get_backend().make_rings(1, max_rows, capacity)
        try:
            manager = CuptiManager(statsMaxLenPerKernel=capacity, rings=rings)
            manager.initialize()
        except BaseException:
            rings.close()
            raise
        cls._rings, cls._cupti_manager = rings, manager

    @classmethod
    def _agree_timing_mode(cls, group) -> None:
        """Once per process group, at the first collective report: the ranks compare how they measure GPU time (one MIN
        all-reduce of a mode code).  Per-kernel keys and per-region keys share no names, so a job in which ONE rank fell
        back to region timing (HIP was up before the import, the tracer could not register, ...) would get NaN for every
        relative GPU score without a word: instead every rank drops to the common mode and says so."""
        import torch
        import torch.distributed as dist

        from . import dist_utils

        mine = _ktrace.mode_code()
        t = torch.tensor([mine, -mine], dtype=torch.int32, device=dist_utils.get_device_for_backend(group))
        dist.all_reduce(t, op=dist.ReduceOp.MIN, group=group)  # (min, -max) in one collective
        common, highest = int(t[0].item()), -int(t[1].item())
        if common == highest:
            _log.info("nvrx straggler: every rank measures GPU time in mode '%s'", _ktrace.timing_mode())
            return
        if common == mine:
            _log.info("nvrx straggler: other ranks of this job trace kernels by name, this one times GPU work per profiled region "
                      "(%s): they fall back to region timing as well", _ktrace.mode_note())
            return
        why = ("another rank of this job cannot trace kernels (its HIP runtime was up before nvrx_straggler was imported, or "
               "the tracer could not register): all ranks time GPU work per profiled region")
        # The agreement is ONE collective per group and is never repeated by a single rank (its peers hold the token and would
        # pair a lone all-reduce with whatever collective they issue next).  What may have to wait is only this rank's own
        # switch: a profiled region is open right now (a report called inside a section) -- it is applied, without any
        # collective, as soon as a report finds no region open (_apply_pending_mode_switch).
        cls._pending_region_switch = why
        cls._apply_pending_mode_switch()

    @classmethod
    def _apply_pending_mode_switch(cls) -> None:
        why = cls._pending_region_switch
        if why is None:
            return
        cls._lane = None  # (the profiler underneath is about to change)
        if cls.cupti_manager.switch_to_regions():
            cls._pending_region_switch = None
            cls._calib, cls._trace_every, cls._trace_gate, cls._trace_sparse = None, 1, True, False  # (region stamps cost next to nothing)
            _ktrace.fall_back_to_regions(why)
            _log.warning("nvrx straggler: %s. GPU scores of THIS report window mix kernel keys and region keys and may be NaN; "
                         "later windows are consistent. Collectives inside profile_cuda sections now count into the region's "
                         "time: keep them outside, or fix the slow-starting rank (NVRX_GPU_TIMING=kernels makes it an error).", why)
        elif not cls._pending_switch_said:
            cls._pending_switch_said = True
            _log.warning("nvrx straggler: %s -- but a profiled region is open on this rank right now (generate_report was called "
                         "inside a detection_section): this rank switches at the first report that finds none open; until then its "
                         "GPU scores are NaN on the other ranks' reports.", why)

    @classmethod
    def shutdown(cls):
        """Undo ``initialize``: wrapped callables get their originals back, profiler, rings and exchange route close."""
        cls._lane = None
        manager, cls._cupti_manager = cls._cupti_manager, None
        if manager is not None:
            manager.shutdown()
        cls.restore_original_callables()
        rings, cls._rings = cls._rings, None
        if rings is not None:
            rings.close()
        reporter = getattr(cls, "reporter", None)
        if reporter is not None:
            reporter.close()
        cls.initialized = False

    # ---- system-side context (not in the reference) --------------------------------------------------
    @classmethod
    def gpu_telemetry(cls) -> dict:
        """Clocks / temperatures / power / utilisation of this rank's GPU from ROCm SMI (``gpu_telemetry.sample``):
        what to look at next to a low individual GPU score.  Raises if ROCm SMI is unavailable."""
        from . import gpu_telemetry

        return gpu_telemetry.sample(_backend_mod.get_backend().device.index)

    @classmethod
    def gpu_telemetry_line(cls) -> str:
        """The same as one log line; never raises."""
        from . import gpu_telemetry

        try:
            index = _backend_mod.get_backend().device.index
        except Exception as e:  # noqa: BLE001
            return f"gpu telemetry unavailable: {e}"
        return gpu_telemetry.describe(index)

    # ---- summaries (host-visible form; the report path itself keeps them on the device) -------------
    @classmethod
    def _get_section_summaries(cls):
        """name -> {Statistic: value} for every section holding samples (computed on the device)."""
        stats = cls.rings.peek_stats()
        out = {}
        for name, section in cls.custom_sections.items():
            if len(section.cpu_elapsed_times) == 0:
                continue
            v = stats[section.row]
            out[name] = {
                Statistic.MIN: float(v[0]), Statistic.MAX: float(v[1]), Statistic.MED: float(v[2]),
                Statistic.AVG: float(v[3]), Statistic.STD: float(v[4]), Statistic.NUM: int(v[5]),
            }
        return out

    @classmethod
    def _get_kernel_summaries(cls):
        """key -> {Statistic: value} for every GPU-timed region (hipEvent rows)."""
        out = {}
        for key, ks in cls.cupti_manager.get_results().items():
            out[key] = {
                Statistic.MIN: ks.min, Statistic.MAX: ks.max, Statistic.MED: ks.median,
                Statistic.AVG: ks.avg, Statistic.STD: ks.stddev, Statistic.NUM: ks.num_calls,
            }
        return out

    @classmethod
    def _reset_sections_elapseds(cls):
        cls.rings.reset()

    # ---- reports -----------------------------------------------------------------------------------
    @classmethod
    def generate_report(cls):
        """Score everything recorded since the last report, then empty the rings.  Collective."""
        assert cls.initialized
        lane = cls._lane
        if lane is not None:
            out = lane.run(cls)
            if out is not _MISS:
                return out
            cls._lane = None  # something it was built on has changed: the general path, and a new lane after it
        report = cls._generate_report_general()
        if cls._lane is None and cls._lanes_enabled:
            cls._lane = _Lane.build(cls)
        return report

    @classmethod
    def _generate_report_general(cls):
        rings = cls.rings
        reporter = cls.reporter
        manager = cls.cupti_manager
        if cls._pending_region_switch is not None:
            cls._apply_pending_mode_switch()
        if reporter.world_size > 1 or cls._mode_agreed is None:
            from . import dist_utils

            world, _ = dist_utils.world_and_rank(reporter.group, reporter._wr_cache)
            token = (world, id(reporter.group)) if world > 1 else "single"
            if token != cls._mode_agreed:
                cls._mode_agreed = token
                if world > 1:
                    cls._agree_timing_mode(reporter.group)
        # the recorded GPU regions must have finished; nothing else on the device is waited for.  Per-kernel tracing:
        # every kernel enqueued inside a section so far has finished and its duration is in its ring (one C call; the
        # tracer's thread has been appending them all along) -- an ASYNCHRONOUS report does not wait even for that:
        # durations that arrive later count in the next window
        if manager.per_kernel and reporter.enqueue_only():
            # ... and what arrives from here to the ring reset below stays with the tracer's thread until then
            manager.cupti_ext.hold(True)
            try:
                manager.harvest(wait=False)
                return cls._report_and_reset(rings, reporter)
            finally:
                manager.cupti_ext.hold(False)
        manager.harvest(wait=True)
        return cls._report_and_reset(rings, reporter)

    @classmethod
    def _report_and_reset(cls, rings, reporter):
        # which rows hold samples this window (one C call); the name tables are rebuilt only when
        # that set changes, so a steady-state report does no per-section Python work
        if rings.occupancy_changed() or cls._occupied_key is not rings:
            counts = rings.counts()
            cls._active_sections = {n: sec.row for n, sec in cls.custom_sections.items() if counts[sec.row] > 0}
            cls._active_kernels = {k: row for k, row in rings.kernel_row_names.items() if counts[row] > 0}
            cls._occupied_key = rings  # (the tables belong to these rings: a re-initialised Detector starts over)
        order_after = _backend_mod.get_backend().current_stream_handle() if reporter.world_size > 1 else None
        report = reporter.generate_report_from_rings(rings, cls._active_sections, cls._active_kernels,
                                                     order_after=order_after)
        keep = reporter.take_unreported_rows() if reporter.asynchronous else None  # (empty unless the report was enqueued on old tables)
        if keep:
            # an asynchronous report that met names it has no ids for ran on the old tables (the ranks sync names at the next
            # report): the samples of those rows were in nobody's report and stay for the next window
            counts = rings.counts()
            keep = [(row, int(counts[row])) for row in keep]
        rings.reset()  # both the section rows and the GPU-time rows, like :241-242 of the reference
        if keep:
            for row, n in keep:
                rings.set_count(row, n)
        return report

    @classmethod
    def generate_report_if_interval_elapsed(cls):
        """Call once per training iteration on every rank; reports when the (rank-synchronised)
        iteration interval has elapsed, otherwise returns None."""
        assert cls.initialized
        tracker = cls.report_interval_tracker
        if cls._calib is not None:
            cls._calibration_mark()
        tracker.iter_increase()
        if cls._calib is not None and tracker.iter_interval is not None:
            cls._calibration_done(tracker.agreed_also)
        return cls.generate_report() if tracker.is_interval_elapsed() else None

    # ---- per-kernel tracing budget -----------------------------------------------------------------
    _MAX_TRACE_EVERY = 64

    @classmethod
    def _calibration_mark(cls) -> None:
        """One call per training iteration while the cost of tracing is being measured -- the interval tracker's 16 timed
        iterations: iterations alternate between tracing the kernels of their profiled sections and not tracing, each one's
        wall time is the distance between two of these calls."""
        marks, flags, enqueued = cls._calib
        # The iteration's DEVICE work has to be inside its wall time: a GPU-bound loop enqueues a step in a fraction of the time the
        # GPU takes for it, and tracing doubles what a launch costs the HOST -- without the wait the host-side times say "tracing
        # costs 266 %" of a loop it slows down by 1.2 % (profiles/r06d_budget_calibration.txt).  Seventeen device
        # synchronisations at the start of a job; the reference synchronises at every report (straggler.py:234).
        try:
            import torch

            if torch.cuda.is_initialized() and torch.cuda.is_available():  # (is_available() re-probes a device-less host: 0.6 s per call)
                torch.cuda.synchronize()
        except RuntimeError:  # (e.g. a stream is being captured into a graph right now: no calibration then)
            cls._calib = None
            cls._trace_gate, cls._trace_sparse = True, cls._trace_every > 1
            return
        marks.append(time.monotonic())
        try:
            enqueued.append(int(cls._cupti_manager.cupti_ext._lib.nvrx_ktrace_counter(0)))  # traced dispatches so far (process-wide)
        except Exception:  # noqa: BLE001  (no tracer underneath: the A/B of the wall times alone decides)
            enqueued.append(0)
        on = len(marks) % 2 == 1  # the iteration that starts now: traced after marks 1, 3, 5 ...
        flags.append(on)
        cls._trace_gate = on
        cls._trace_sparse = (not on) or cls._trace_every > 1

    @classmethod
    def _trace_every_needed(cls) -> float:
        """What the interval tracker's all-reduce carries for this rank (``ReportIntervalTracker.also_max``): the multiple of
        ``profiling_interval`` at which tracing fits the budget, from the medians of the traced and the untraced iterations."""
        if cls._calib is None:
            return 1.0
        marks, flags, enqueued = cls._calib
        steps = [b - a for a, b in zip(marks, marks[1:])]
        t_on = sorted(t for t, f in zip(steps, flags) if f)
        t_off = sorted(t for t, f in zip(steps, flags) if not f)
        traced = sorted(b - a for a, b, f in zip(enqueued, enqueued[1:], flags) if f)
        cls.kernel_trace_cost_pct = None
        if not t_on or not t_off:
            return 1.0
        if cls.profiling_interval == 1:
            m_on, m_off = t_on[(len(t_on) - 1) // 2], t_off[(len(t_off) - 1) // 2]  # lower medians, as the tracker's
        else:
            # only every profiling_interval-th entry is traced at all, so only some of the "traced" iterations carry the cost:
            # the average is what a step pays (less robust than a median; the default interval is 1)
            m_on, m_off = sum(t_on) / len(t_on), sum(t_off) / len(t_off)
        if m_off <= 0.0:
            return 1.0
        cost = (m_on - m_off) / m_off * 100.0
        # Second estimate, from what CAN be measured exactly in 16 iterations: the number of dispatches a traced iteration
        # had, times what one traced dispatch costs the GPU.  That cost is rocprofiler-sdk's completion signal and timestamps:
        # 0.3-1.6 us per dispatch on the eleven boxes of rounds 5-6 (docs/MEASUREMENTS.md), 1.0 us assumed.  The A/B above
        # resolves a launch-bound loop's overhead (tracing doubles what a launch costs the host: tens of per cent) but not one
        # per cent of a GPU-bound step from eight iterations each way (a box where the paired A/B of 140 steps says 1.4 %
        # measured 0.03 % here, profiles/r06y_bench_driver.json); the larger estimate decides.
        if traced:
            n = traced[(len(traced) - 1) // 2]
            cls.kernel_trace_dispatches = int(n)
            model = n * _TRACED_DISPATCH_US * 1e-6 / m_off * 100.0
            if cls.profiling_interval > 1:
                model = sum(traced) / len(traced) * _TRACED_DISPATCH_US * 1e-6 / m_off * 100.0
            cost = max(cost, model)
        cls.kernel_trace_cost_pct = cost
        if cost <= cls.kernel_trace_budget_pct:
            return 1.0
        return float(min(cls._MAX_TRACE_EVERY, int(-(-cost // cls.kernel_trace_budget_pct))))

    @classmethod
    def _calibration_done(cls, agreed: Optional[float]) -> None:
        """The ranks take the LARGEST multiple any of them needs (kernel summaries are compared across ranks: they should
        cover the same share of the entries); it came back with the interval tracker's own all-reduce."""
        mine = int(cls._trace_every_needed())
        cost, n = cls.kernel_trace_cost_pct, len(cls._calib[0]) - 1
        disp = cls.kernel_trace_dispatches
        cls._calib = None
        every = max(1, min(cls._MAX_TRACE_EVERY, int(agreed))) if agreed else mine
        cls._trace_every, cls._trace_gate = every, True
        cls._trace_sparse = every > 1
        total = cls.profiling_interval * every
        _log.info("nvrx straggler: tracing the kernels of the profiled sections costs this rank %s of an iteration at "
                  "profiling_interval=%d (the larger of: %s of %d iterations with and %d without; %s traced dispatches x 1 us); budget %.2f %%: kernels are traced on every "
                  "%d%s entry of a profile_cuda section%s", "%.2f %%" % cost if cost is not None else "an unmeasured share",
                  cls.profiling_interval, "medians" if cls.profiling_interval == 1 else "means", (n + 1) // 2, n // 2,
                  "?" if disp is None else disp, cls.kernel_trace_budget_pct, total,
                  {1: "st", 2: "nd", 3: "rd"}.get(total if total < 20 else total % 10, "th"),
                  "" if every == mine else " (another rank needed the larger interval)")

    @classmethod
    def is_interval_elapsed(cls) -> bool:
        return cls.report_interval_tracker.is_interval_elapsed()

    # ---- sections ----------------------------------------------------------------------------------
    @staticmethod
    def _get_this_context_block_location() -> str:
        # frames: this function <- detection_section generator <- contextmanager.__enter__ <- user code
        frame = sys._getframe(3)
        return f"{frame.f_code.co_filename}:{frame.f_lineno}"

    @classmethod
    def _ensure_section_name_is_valid(cls, name, location):
        known = cls.custom_sections.get(name)
        if known is not None and known.location != location:
            raise ValueError(f"Section name '{name}' is already used at: {known.location}")

    @classmethod
    @contextmanager
    def detection_section(cls, name: Optional[str] = None, profile_cuda: bool = True):
        """Time the enclosed block.

        Args:
            name: section name for reports (default: ``file:line`` of the ``with`` statement).
            profile_cuda: also measure the block's GPU time with a hipEvent pair on the current
                stream; it feeds the rank's GPU performance score.
        """
        if not cls.initialized:
            raise RuntimeError("Detector is not initialized.")

        section = cls.custom_sections.get(name) if name is not None else None
        if section is None:
            location = cls._get_this_context_block_location()
            if name is None:
                name = location
            section = cls.custom_sections.get(name)
            if section is None:
                section = CustomSection(name=name, location=location, rings=cls.rings)
                cls.custom_sections[name] = section

        profiled = (section.total_entry_cnt % cls.profiling_interval) == 0
        section.total_entry_cnt += 1
        if not profiled:
            yield
            return

        if profile_cuda and cls._trace_sparse:
            # the tracing budget (initialize: kernel_trace_budget_pct): this entry's wall time is recorded, its kernels are traced
            # only on every (profiling_interval x _trace_every)-th entry -- and not at all in the untraced calibration iterations
            profile_cuda = cls._trace_gate and ((section.total_entry_cnt - 1) // cls.profiling_interval) % cls._trace_every == 0
        if profile_cuda:
            cls.cupti_manager.start_profiling(GPU_KEY_PREFIX + name)
        t0 = time.perf_counter_ns()
        try:
            yield
        except BaseException:
            # no sample for an entry that raised; just close the GPU region
            if profile_cuda:
                cls.cupti_manager.stop_profiling()
            raise
        elapsed_ms = (time.perf_counter_ns() - t0) * 1e-6
        # with device timestamps the kernel that closes the GPU region also appends this sample
        if not (profile_cuda and cls.cupti_manager.stop_profiling(section.row, elapsed_ms)):
            cls.rings.push(section.row, elapsed_ms)

    # ---- callable wrapping -------------------------------------------------------------------------
    @classmethod
    def _build_wrapper(cls, fn, callable_id, profile_cuda: bool = True):
        """``fn`` run inside the section named after ``callable_id``."""
        section = functools.partial(cls.detection_section, name=str(callable_id), profile_cuda=profile_cuda)

        @functools.wraps(fn)
        def timed(*args, **kwargs):
            with section():
                return fn(*args, **kwargs)

        return timed

    @classmethod
    def wrap_callables(cls, callable_ids: List[CallableId], profile_cuda: bool = True):
        """Replace each ``getattr(cid.obj, cid.name)`` by a version that runs inside
        ``detection_section(str(cid))``."""
        cls.original_callables = {cid: getattr(cid.obj, cid.name) for cid in callable_ids}
        for cid, original in cls.original_callables.items():
            setattr(cid.obj, cid.name, cls._build_wrapper(original, cid, profile_cuda=profile_cuda))

    @classmethod
    def restore_original_callables(cls):
        for cid, original in (cls.original_callables or {}).items():
            setattr(cid.obj, cid.name, original)
