"""Compute backend of the straggler path: the HIP engine, and nothing else.

``get_backend()`` returns the process-wide :class:`HipBackend`.  Constructing it requires the in-tree
``libnvrx_straggler_hip.so`` and a visible MI355X; otherwise it raises -- there is no CPU fallback in
the product.  ``set_backend()`` exists so the CPU-only unit tests can inject their own checker
backend (built on ``oracle/``, which lives outside this package) to exercise the host-side logic
(name mapping, exchange, report assembly, Detector plumbing) on a box without a GPU.

Data layout in HBM (all f32 unless noted; see include/nvrx_straggler.h):

* rings   ``[local_ranks * rows_per_rank][row_stride]``  one timing row per section / GPU-timed region
* stats   ``[rows][8]``        MIN MAX MED AVG STD NUM WEIGHT pad
* send    ``[local_ranks][L]`` this GPU's exchange rows, ``L = 2(K+S) + K + 1``
* table   ``[R][L]``           all ranks' rows after the all-gather
* scores  ``[R][2+2S]``, flags ``[R][2+2S]`` u8, meta ``[4]`` u32

``meta | scores | flags | stats`` live in ONE device allocation mirrored by ONE pinned host buffer, so
a report needs a single small D2H copy.
"""
from __future__ import annotations

import ctypes
import os
import threading
import weakref
from typing import Any, Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _native
from .row_families import EPISODE, FAMILIES, ONSET, PERIOD, TAIL, RowFamily
from .table_families import NODE, PACE, PACE_GROUP, PEER, ROBUST, SLOTS, TableFamily

DEFAULT_THRESHOLDS = (0.75, 0.75, 0.75, 0.75)  # gpu_rel, section_rel, gpu_indiv, section_indiv



def report_timeout_s() -> float:
    """How long a report waits for its completion word.  The score kernel is queued behind the report's
    collective, so this bounds how late the slowest PEER may reach ``generate_report`` (first-report RCCL set-up,
    a checkpoint or evaluation on one rank, an actual straggler).  The reference simply blocks in its collective
    until the process group's timeout; the default here is c10d's 30 minutes.  ``NVRX_REPORT_TIMEOUT_S`` overrides
    it, ``0`` waits for ever."""
    t = _timeout_cache[0]
    if t is None:
        t = refresh_report_timeout()
    return t


_timeout_cache = [None]  # read once: a report (and the wait for the previous asynchronous one) does not look at the environment


def refresh_report_timeout() -> float:
    """Re-read ``NVRX_REPORT_TIMEOUT_S`` (a process that changes it after its first report calls this)."""
    try:
        t = float(os.environ.get("NVRX_REPORT_TIMEOUT_S", "1800"))
    except ValueError:
        t = 1800.0
    _timeout_cache[0] = t
    return t


_backend = None
_backend_lock = threading.Lock()

# torch.cuda.current_stream() builds a Stream object through several Python layers (~3 us); the raw
# handle is one C call.  Private API, so fall back to the public one if it ever goes away.
_raw_stream_fn = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _raw_current_stream(device_index: int) -> int:
    if _raw_stream_fn is not None:
        return _raw_stream_fn(device_index)
    return torch.cuda.current_stream(device_index).cuda_stream


def set_backend(backend) -> None:
    """Install a backend object (tests only; pass ``None`` to go back to the HIP engine)."""
    global _backend
    with _backend_lock:
        _backend = backend


_NO_DEVICE = ("nvrx_straggler: no HIP device is visible (torch.cuda.is_available() is False). "
              "The MI355X straggler-scoring path has no CPU fallback.")


def require_engine() -> None:
    """Fail NOW where the engine cannot run (library not built, no HIP device) -- without creating it: the engine binds to
    the device that is current when it is first used, which a script may select only after ``Detector.initialize``."""
    if _backend is not None:
        return
    _native.load()
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_DEVICE)


def get_backend():
    """The active backend; creates the HIP engine on first use and fails loudly if it cannot."""
    global _backend
    if _backend is None:
        with _backend_lock:
            if _backend is None:
                _backend = HipBackend()
    return _backend


def _nobody():
    """A dead weak reference."""
    return None


def _align(n: int, a: int = 64) -> int:
    return (n + a - 1) // a * a


class ResultBlock:
    """One result block in PINNED, device-mapped host memory: ``meta | scores | flags | stats``.  The kernels store their
    results straight into it and the score kernel publishes a sequence word last (``meta[4]``; ``meta[5]`` for the
    statistics rows, which a resident score kernel forwards after the scores), so a report needs no D2H copy and no
    stream synchronisation.  A workspace owns TWO of them and alternates: the block of report n is not written again
    before report n+2, so a caller that still holds report n while it asks for n+1 (``report = generate_report()`` in
    a loop does exactly that) costs the next report nothing -- with one block the next report first had to wait for
    the previous one's statistics rows and copy 16 KB out of the way."""

    def __init__(self, ws: "Workspace", backend: "HipBackend"):
        R, W, stats_rows = ws.R, ws.W, ws.stats_rows
        self._off_meta = 0
        self._off_scores = self._off_meta + _align(_native.META_WORDS * 4)
        self._off_flags = self._off_scores + _align(R * W * 4)
        self._off_stats = self._off_flags + _align(R * W)
        self.nbytes = self._off_stats + _align(max(stats_rows, 1) * _native.STATS_STRIDE * 4)
        h_ptr, d_ptr = ctypes.c_void_p(), ctypes.c_void_p()
        _native.check(backend.lib.nvrx_host_alloc(ctypes.byref(h_ptr), ctypes.byref(d_ptr), self.nbytes))
        self._lib = backend.lib
        self._backend = backend
        self.h_ptr, self.d_ptr = h_ptr.value, d_ptr.value
        host = np.frombuffer((ctypes.c_uint8 * self.nbytes).from_address(self.h_ptr), dtype=np.uint8)
        self._host = host
        self.stats = host[self._off_stats : self._off_stats + stats_rows * 32].view(np.float32).reshape(stats_rows, _native.STATS_STRIDE)
        self.meta = host[self._off_meta : self._off_meta + _native.META_WORDS * 4].view(np.uint32)
        # the same words without numpy (a scalar read of the pinned block through numpy costs a report microseconds when cold)
        self.meta_words = (ctypes.c_uint32 * _native.META_WORDS).from_address(self.h_ptr + self._off_meta)
        self.scores = host[self._off_scores : self._off_scores + R * W * 4].view(np.float32).reshape(R, W)
        self.flags = host[self._off_flags : self._off_flags + R * W].reshape(R, W)
        self.h_stats_dst = self.d_ptr + self._off_stats
        self.d_meta = self.d_ptr + self._off_meta
        self.d_scores = self.d_ptr + self._off_scores
        self.d_flags = self.d_ptr + self._off_flags
        self.h_seq = self.h_ptr + self._off_meta + 16  # meta[4]: scores / flags / meta have landed
        self.h_seq2 = self.h_ptr + self._off_meta + 20  # meta[5]: the statistics rows have landed
        # descriptor of the one-call report (nvrx_report) into THIS block; the library advances desc.seq itself
        d = self.desc = _native.ReportDesc()
        d.R, d.K, d.S = ws.R, ws.K, ws.S
        d.names_ok, d.rows_active, d.do_indiv, d.do_rel, d.stats_rows = 1, 0, 1, 1, 0
        for i, t in enumerate(DEFAULT_THRESHOLDS):
            d.thresholds[i] = t
        d.d_stats, d.d_send, d.d_table = ws.d_stats, ws.send_ptr, ws.table_ptr
        d.d_scores, d.d_flags, d.d_meta, d.d_stats_dst = self.d_scores, self.d_flags, self.d_meta, self.h_stats_dst
        d.d_done_counter = ws.d_counter
        d.allgather_fn, d.comm, d.send_count = None, None, ws.local_ranks * ws.L
        d.seq = 0
        d.h_seq_word = self.h_seq
        d.timeout_s = report_timeout_s()
        self.desc_ref = ctypes.byref(d)
        self.desc_key = None
        # this block's last report may still be "live" (read lazily by a Report): see attach() / settle()
        self._live = None
        self._live_seq = 0

    def free(self) -> None:
        if self.h_ptr:
            self._lib.nvrx_host_free(self.h_ptr)
            self.h_ptr = None

    def attach(self, live) -> None:
        """``live`` (reporting._LiveBlock) reads this block lazily; ``settle()`` collects it before the block is reused."""
        self._live = weakref.ref(live)
        self._live_seq = live.seq

    def mark_live(self, seq: int) -> None:
        """A one-call report with sequence number ``seq`` ran on this block and nobody may be holding it (a rank that
        returns ``None``, a report abandoned for a name sync): ``settle()`` still has to see its statistics rows land."""
        self._live = _nobody
        self._live_seq = seq

    def settle(self) -> None:
        """Called before anything is enqueued that writes this block again: its last report's statistics rows must have
        landed (a resident score kernel forwards them after the scores), and if somebody still holds that report its data
        is copied out now."""
        ref = self._live
        if ref is not None:
            self._live = None
            live = ref()
            if live is not None:
                live.detach()
            elif self.meta_words[5] != self._live_seq:
                self._backend.wait_seq(None, self._live_seq, stats=True, block=self)

    def host_block(self) -> np.ndarray:
        """A private copy of the whole block (the block itself is overwritten two reports later)."""
        return self._host.copy()

    def host_head(self) -> np.ndarray:
        """A private copy of meta | scores | flags (valid once meta[4] shows the report's sequence number)."""
        return self._host[: self._off_stats].copy()

    def host_head_bytes(self) -> bytes:
        """The same as ``bytes``: one memcpy out of the pinned block, no numpy object involved."""
        return ctypes.string_at(self.h_ptr, self._off_stats)

    def host_stats(self, rows: int) -> np.ndarray:
        """A private copy of the first ``rows`` statistics rows (valid once meta[5] shows the sequence number)."""
        return self.stats[:rows].copy()


class Attribution:
    """Kernel attribution of one report (``nvrx_attribute`` / ``nvrx_report_attribute``), enqueued and not waited for: the
    records -- ``[n_ranks][2 families][1 + top_n][4]`` 32-bit words, include/nvrx_straggler.h -- are in the workspace's device
    buffer once the kernel has run.  ``records()`` waits for it and takes the private host copy (one ordered D2H on the
    backend's stream): when a ``Report`` first asks, or -- ``Workspace.attr_settle`` -- before the next report on the same
    workspace rewrites the table the kernel reads and the buffer it writes."""

    __slots__ = ("backend", "d_ptr", "first_rank", "n_ranks", "top_n", "_host", "_lock", "_keep")

    def __init__(self, backend: "HipBackend", buf: torch.Tensor, first_rank: int, n_ranks: int, top_n: int):
        self.backend, self.d_ptr = backend, buf.data_ptr()
        self.first_rank, self.n_ranks, self.top_n = first_rank, n_ranks, top_n
        self._host: Optional[np.ndarray] = None
        self._lock = threading.Lock()
        self._keep = buf  # the device buffer lives at least until the copy is taken

    def records(self) -> np.ndarray:
        """``[n_ranks, 2, 1 + top_n, 4]`` uint32 (private copy); the first call waits for the kernel."""
        if self._host is None:
            with self._lock:
                if self._host is None:
                    self._host = self.backend.attribution_copy_out(self)
                    self.backend = self._keep = None
        return self._host


class RowScores:
    """One row family's scores of one report (``nvrx_<family>_local`` -> exchange -> ``nvrx_<family>_score``;
    row_families.py), enqueued and not waited for: once the score kernel has run, the workspace's buffer of that family
    holds the gathered table ``[R][P][K+S]`` (``[R][K+S]`` for a family of one plane) and, behind it, the scores
    ``[n_ranks][1 + S]`` of the reported ranks.  ``records()`` waits for it and takes the private host copy (one ordered D2H
    on the backend's stream): when a ``Report`` first asks, or -- ``Workspace.family_settle`` -- before the next report on
    the same workspace rewrites the table the kernel reads and the buffers it writes."""

    __slots__ = ("backend", "family", "d_ptr", "R", "K", "S", "first_rank", "n_ranks", "params", "_host", "_lock", "_keep")

    def __init__(self, backend: "HipBackend", family: RowFamily, buf: torch.Tensor, R: int, K: int, S: int, first_rank: int,
                 n_ranks: int, params: tuple = ()):
        self.backend, self.family, self.d_ptr = backend, family, buf.data_ptr()
        self.R, self.K, self.S = R, K, S
        self.first_rank, self.n_ranks, self.params = first_rank, n_ranks, params
        self._host = None
        self._lock = threading.Lock()
        self._keep = buf  # the device buffer lives at least until the copy is taken

    def records(self):
        """``(planes [n_ranks, P, K+S], scores [n_ranks, 1 + S])`` f32 of the reported ranks -- ``[n_ranks, K+S]`` for a
        family of one plane -- (private copies); the first call waits for the kernels."""
        if self._host is None:
            with self._lock:
                if self._host is None:
                    self._host = getattr(self.backend, self.family.stem + "_copy_out")(self)
                    self.backend = self._keep = None
        return self._host


class RowGroupScores(RowScores):
    """One row family's scores per peer group of one report (``nvrx_rowfam_group_score``), ``RowScores``' sibling in the same
    slot: once the kernels have run, the workspace's buffer of that family holds the gathered table, then -- on a 16-byte
    boundary -- the ``[G][K+S]`` column records and the scores ``[n_ranks][1 + S]`` of the reported ranks.  ``records()`` waits
    for them and takes the private host copy by one ordered D2H, as ``RowScores.records`` does."""

    __slots__ = ("G", "min_ranks")

    def __init__(self, backend: "HipBackend", family: RowFamily, buf: torch.Tensor, R: int, K: int, S: int, G: int,
                 first_rank: int, n_ranks: int, min_ranks: int, params: tuple = ()):
        super().__init__(backend, family, buf, R, K, S, first_rank, n_ranks, params)
        self.G, self.min_ranks = G, min_ranks

    def records(self):
        """``(planes, scores, cols)``: ``RowScores.records``' two arrays and the column records ``[G, K+S, 4]`` uint32 {f32
        floor, u32 present, i32 floor_rank, u32 members} (private copies); the first call waits for the kernels."""
        if self._host is None:
            with self._lock:
                if self._host is None:
                    self._host = self.backend.family_group_copy_out(self)
                    self.backend = self._keep = None
        return self._host


class _FamilyBuffers:
    """A workspace's device buffers of one row family, and the handle that may still be using them."""

    __slots__ = ("buf", "send", "table", "scratch", "last")


class TableScores:
    """One table family's scores of one report (``nvrx_<family>_score`` / ``nvrx_report_<family>``; table_families.py),
    enqueued and not waited for: once the kernels have run, the family's slot of the workspace holds its block of 32-bit
    words (include/nvrx_straggler.h).  ``records()`` waits for them and takes the private host copy (one ordered D2H on the
    backend's stream): when a ``Report`` first asks, or -- ``Workspace.table_settle`` -- before the next report on the same
    workspace rewrites the table the kernels read and the buffer they write.  ``G`` is 0 for a job-wide family; the family's
    parameters (``min_ranks``, ``floor_rel``, ...) read as attributes."""

    __slots__ = ("backend", "family", "d_ptr", "G", "K", "S", "first_rank", "n_ranks", "params", "_host", "_lock", "_keep")

    def __init__(self, backend: "HipBackend", family: TableFamily, buf: torch.Tensor, G: int, K: int, S: int, first_rank: int,
                 n_ranks: int, params: tuple):
        self.backend, self.family, self.d_ptr = backend, family, buf.data_ptr()
        self.G, self.K, self.S = G, K, S
        self.first_rank, self.n_ranks, self.params = first_rank, n_ranks, params
        self._host = None
        self._lock = threading.Lock()
        self._keep = buf  # the device buffer lives at least until the copy is taken

    def __getattr__(self, name):  # (only what the slots do not have: the family's parameters by name)
        names = object.__getattribute__(self, "family").params
        if name in names:
            return self.params[names.index(name)]
        raise AttributeError(name)

    def records(self):
        """The family's arrays (``TableFamily.blocks``: private copies); the first call waits for the kernels."""
        if self._host is None:
            with self._lock:
                if self._host is None:
                    self._host = getattr(self.backend, self.family.name + "_copy_out")(self)
                    self.backend = self._keep = None
        return self._host


class _TableBuffers:
    """A workspace's records buffer of one table-family slot, and the handle that may still be using it."""

    __slots__ = ("buf", "last")


class PeerGroups:
    """The peer groups of one ``ReportGenerator``, resolved for a table of ``R`` logical ranks: ``labels`` in order of first
    appearance by ascending rank (their positions are the dense group ids), and the array ``nvrx_peer_score`` takes --
    ``group[R] | members[R] | start[G+1]`` int32 (include/nvrx_straggler.h) -- on the host and, uploaded once under the
    backend's stream by the backend that first asks, on the device."""

    __slots__ = ("R", "G", "labels", "host", "_dev", "_max_size")

    def __init__(self, rank_labels: Sequence[Any]):
        self.R = len(rank_labels)
        ids: Dict[Any, int] = {}
        group = np.fromiter((ids.setdefault(lab, len(ids)) for lab in rank_labels), dtype=np.int32, count=self.R)
        self.labels = tuple(ids)
        self.G = len(ids)
        if self.G > _native.PEER_MAX_GROUPS:
            raise ValueError(f"peer_groups: {self.G} groups, at most {_native.PEER_MAX_GROUPS}")
        members = np.argsort(group, kind="stable").astype(np.int32)  # by (group id, rank)
        start = np.zeros(self.G + 1, dtype=np.int32)
        np.cumsum(np.bincount(group, minlength=self.G), out=start[1:])
        self.host = np.concatenate((group, members, start))
        self._dev = None
        self._max_size = None

    @classmethod
    def resolve(cls, spec, R: int, what: str = "peer_groups") -> "PeerGroups":
        """``spec`` as ``ReportGenerator`` keeps it -- ``("block", N)``, ``("mod", N)`` or a tuple of labels, one per
        logical rank -- for a table of ``R`` ranks (``what``: the option's name in the message)."""
        if isinstance(spec, _PeerRule):
            kind, n = spec
            return cls([r // n if kind == "block" else r % n for r in range(R)])
        if len(spec) != R:
            raise ValueError(f"{what} has {len(spec)} labels, the job has {R} logical ranks")
        return cls(spec)

    @property
    def group(self) -> np.ndarray:
        return self.host[: self.R]

    @property
    def max_size(self) -> int:
        """The largest group's size (``nvrx_pace_group_score``'s ``max_group``; worked out when first asked for)."""
        if self._max_size is None:
            self._max_size = int(np.diff(self.host[2 * self.R :]).max())
        return self._max_size

    def members(self, g: int) -> List[int]:
        start = self.host[2 * self.R :]
        return self.host[self.R + start[g] : self.R + start[g + 1]].tolist()

    def device(self, backend: "HipBackend") -> torch.Tensor:
        if self._dev is None:
            with torch.cuda.stream(backend.stream):  # (allocated, written and read under the backend's stream)
                self._dev = torch.from_numpy(self.host).to(backend.device)
        return self._dev


class _PeerRule(tuple):
    """``("block", N)`` / ``("mod", N)``: a rule that yields the labels once the number of ranks is known (a plain tuple is a
    list of labels)."""


class ScoreHistory:
    """The score history of one ``ReportGenerator`` (``nvrx_score_history`` / ``nvrx_report_history``): the ring of the last
    ``depth`` reports' scores -- ``hist``, f32 ``[n_ranks][2][1 + S_cap][stride]`` where the backend keeps it, NaN where
    nothing was appended --, the number of reports appended so far and the section ids the ring has room for.  The backend
    that runs the step allocates and grows ``hist`` (``HipBackend.score_history``); the state itself only says when the
    history starts again: a change of the reported ranks, or ``reset()``."""

    __slots__ = ("depth", "stride", "hist", "S_cap", "n_before", "ranks")

    def __init__(self, depth: int):
        self.depth, self.stride = int(depth), _native.history_stride(int(depth))
        self.reset()

    def reset(self) -> None:
        self.hist, self.S_cap, self.n_before, self.ranks = None, 0, 0, None

    def begin(self, first_rank: int, n_ranks: int) -> None:
        """A step for ranks ``[first_rank, first_rank + n_ranks)`` is about to run: another range than last time starts the
        history again."""
        if self.ranks != (first_rank, n_ranks):
            self.reset()
            self.ranks = (first_rank, n_ranks)

    @staticmethod
    def capacity(S: int) -> int:
        """Section ids a ring that has to hold ``S`` is given room for: the next multiple of 64."""
        return max(64, -(-S // 64) * 64)


class PeerHistory(ScoreHistory):
    """The peer-score history of one ``ReportGenerator`` (``nvrx_peer_history`` / ``nvrx_report_peer_history``): a
    ``ScoreHistory`` whose ring holds the peer step's scores -- one family, ``hist`` f32 ``[n_ranks][1 + S_cap][stride]`` --
    and whose ``n_before`` counts the reports for which the peer step ran on this rank."""

    __slots__ = ()


class History:
    """The score history after one report (``nvrx_score_history`` / ``nvrx_report_history``), enqueued and not waited for: once
    the kernel has run, the workspace's device buffer holds ``[n_ranks][2][1 + S][8]`` 32-bit words ``{latest, median, worst,
    best, streak, below, present, depth}`` (include/nvrx_straggler.h).  ``records()`` waits for it and takes the private host
    copy (one ordered D2H on the backend's stream): when a ``Report`` first asks, or -- ``Workspace.history_settle`` --
    before the next report on the same workspace rewrites the block the kernel read and the buffer it wrote.  ``fams``: 2, or
    1 for the peer-score history (``nvrx_peer_history``: ``[n_ranks][1][1 + S][8]``, settled by
    ``Workspace.peer_history_settle``)."""

    __slots__ = ("backend", "d_ptr", "S", "first_rank", "n_ranks", "fams", "_host", "_lock", "_keep")

    def __init__(self, backend: "HipBackend", buf: torch.Tensor, S: int, first_rank: int, n_ranks: int, fams: int = 2):
        self.backend, self.d_ptr = backend, buf.data_ptr()
        self.S, self.first_rank, self.n_ranks, self.fams = S, first_rank, n_ranks, fams
        self._host = None
        self._lock = threading.Lock()
        self._keep = buf  # the device buffer lives at least until the copy is taken

    def records(self) -> np.ndarray:
        """``[n_ranks, fams, 1 + S, 8]`` uint32 (private copy); the first call waits for the kernel."""
        if self._host is None:
            with self._lock:
                if self._host is None:
                    self._host = self.backend.history_copy_out(self)
                    self.backend = self._keep = None
        return self._host


class Trend:
    """The score trends after one report (``nvrx_score_trend`` / ``nvrx_report_trend``), enqueued and not waited for: once the
    kernel has run, the workspace's device buffer holds ``[n_ranks][2][1 + S][4]`` 32-bit words ``{slope, level, S, usable}``
    (include/nvrx_straggler.h).  ``records()`` waits for it and takes the private host copy (one ordered D2H on the backend's
    stream): when a ``Report`` first asks, or -- ``Workspace.trend_settle`` -- before the next trend step on the same
    workspace rewrites the buffer.  ``fams``: 2, or 1 for the peer-score trends (``nvrx_peer_trend``: ``[n_ranks][1][1 + S][4]``,
    settled by ``Workspace.peer_trend_settle``)."""

    __slots__ = ("backend", "d_ptr", "S", "n_ranks", "fams", "_host", "_lock", "_keep")

    def __init__(self, backend: "HipBackend", buf: torch.Tensor, S: int, n_ranks: int, fams: int = 2):
        self.backend, self.d_ptr = backend, buf.data_ptr()
        self.S, self.n_ranks, self.fams = S, n_ranks, fams
        self._host = None
        self._lock = threading.Lock()
        self._keep = buf  # the device buffer lives at least until the copy is taken

    def records(self) -> np.ndarray:
        """``[n_ranks, fams, 1 + S, 4]`` uint32 (private copy); the first call waits for the kernel."""
        if self._host is None:
            with self._lock:
                if self._host is None:
                    self._host = self.backend.trend_copy_out(self)
                    self.backend = self._keep = None
        return self._host


class Slack:
    """The slack scores of one report (``nvrx_slack_score``), enqueued and not waited for: once the kernels have run, the
    workspace's device buffer holds the job record, the 64 column records and every rank's record (include/
    nvrx_straggler.h).  ``records()`` waits for them and takes the private host copy (one ordered D2H on the backend's stream):
    when a ``Report`` first asks, or -- ``Workspace.slack_settle`` -- before the next slack step on the same workspace
    rewrites the buffers."""

    __slots__ = ("backend", "d_ptr", "first_rank", "n_ranks", "min_ranks", "_host", "_lock", "_keep")

    def __init__(self, backend: "HipBackend", buf: torch.Tensor, first_rank: int, n_ranks: int, min_ranks: int):
        self.backend, self.d_ptr = backend, buf.data_ptr()
        self.first_rank, self.n_ranks, self.min_ranks = first_rank, n_ranks, min_ranks
        self._host = None
        self._lock = threading.Lock()
        self._keep = buf  # the device buffer lives at least until the copy is taken

    def records(self):
        """``(job [8], columns [64, 4], ranks [n_ranks, 8])`` uint32 (private copies), the ranks being ``[first_rank,
        first_rank + n_ranks)``; the first call waits for the kernels."""
        if self._host is None:
            with self._lock:
                if self._host is None:
                    self._host = self.backend.slack_copy_out(self)
                    self.backend = self._keep = None
        return self._host


class SlackGroup:
    """The slack scores per peer group of one report (``nvrx_slack_group_score``), enqueued and not waited for: ``Slack``'s
    sibling, in the same slot of the workspace (``Workspace.slack_buffers`` / ``slack_settle``: a report runs one of the
    two).  Once the kernels have run, the device buffer holds the ``G`` group records, the ``G x 64`` pair records and every
    rank's record (include/nvrx_straggler.h)."""

    __slots__ = ("backend", "d_ptr", "G", "first_rank", "n_ranks", "min_ranks", "min_peers", "_host", "_lock", "_keep")

    def __init__(self, backend: "HipBackend", buf: torch.Tensor, G: int, first_rank: int, n_ranks: int, min_ranks: int,
                 min_peers: int):
        self.backend, self.d_ptr, self.G = backend, buf.data_ptr(), G
        self.first_rank, self.n_ranks, self.min_ranks, self.min_peers = first_rank, n_ranks, min_ranks, min_peers
        self._host = None
        self._lock = threading.Lock()
        self._keep = buf  # the device buffer lives at least until the copy is taken

    def records(self):
        """``(groups [G, 8], pairs [G, 64, 4], ranks [n_ranks, 8])`` uint32 (private copies), the ranks being ``[first_rank,
        first_rank + n_ranks)``; the first call waits for the kernels."""
        if self._host is None:
            with self._lock:
                if self._host is None:
                    self._host = self.backend.slack_group_copy_out(self)
                    self.backend = self._keep = None
        return self._host


class Work:
    """The work groups of one report (``nvrx_work_groups`` / ``nvrx_report_work``), enqueued and not waited for: once the four
    kernels have run, the workspace's device buffer holds the block of include/nvrx_straggler.h -- signatures, adjacency,
    partial nearest records, rank records, job record.  ``records()`` waits for them and takes the private host copy of the
    rank records and the job record (one ordered D2H on the backend's stream): when a ``Report`` first asks, when
    ``peer_groups="auto"`` needs the groups, or -- ``Workspace.work_settle`` -- before the next report on the same workspace
    rewrites the table the kernels read and the buffer they write."""

    __slots__ = ("backend", "d_ptr", "R", "K", "S", "count_tol", "max_unlike_ppm", "_host", "_lock", "_keep")

    def __init__(self, backend: "HipBackend", buf: torch.Tensor, R: int, K: int, S: int, count_tol: float, max_unlike_ppm: int):
        self.backend, self.d_ptr = backend, buf.data_ptr()
        self.R, self.K, self.S = R, K, S
        self.count_tol, self.max_unlike_ppm = count_tol, max_unlike_ppm
        self._host = None
        self._lock = threading.Lock()
        self._keep = buf  # the device buffer lives at least until the copy is taken

    def records(self):
        """``(ranks [R, 8], job [4])`` uint32 (private copies): ``{root, size, degree, nearest, nearest_unlike, nearest_either,
        kernels_present, sections_present}`` per rank and ``{groups, singletons, largest, ranks_with_data}``; the first call
        waits for the kernels."""
        if self._host is None:
            with self._lock:
                if self._host is None:
                    self._host = self.backend.work_copy_out(self)
                    self.backend = self._keep = None
        return self._host


class Workspace:
    """Buffers of one report shape (R ranks, K kernel ids, S section ids): the exchange rows and the gathered table in
    device memory, and two result blocks (``ResultBlock``) that successive reports alternate between.  ``ws.meta /
    scores / flags / stats`` are those of the CURRENT block, i.e. of the report that ran last."""

    def __init__(self, backend: "HipBackend", R: int, K: int, S: int, local_ranks: int, stats_rows: int):
        self.R, self.K, self.S = R, K, S
        self.local_ranks = local_ranks
        self.stats_rows = stats_rows
        self.L = _native.table_len(K, S)
        self.W = _native.score_len(S)
        dev = backend.device
        self.send = torch.empty((local_ranks, self.L), dtype=torch.float32, device=dev)
        self.table = torch.empty((R, self.L), dtype=torch.float32, device=dev) if R != local_ranks else self.send
        self.send_initialised = False
        # statistics are produced in device memory and forwarded to the host block by the score kernel
        self.stats_dev = torch.zeros((max(stats_rows, 1), _native.STATS_STRIDE), dtype=torch.float32, device=dev)
        self.d_stats = self.stats_dev.data_ptr()
        self.done_counter = torch.zeros(1, dtype=torch.int32, device=dev)
        self.d_counter = self.done_counter.data_ptr()
        self.seq = 0  # the one sequence every report on this workspace draws from, whichever block and route it takes
        self.send_ptr = self.send.data_ptr()
        self.table_ptr = self.table.data_ptr()
        self._backend = backend
        self.blocks = (ResultBlock(self, backend), ResultBlock(self, backend))
        self.block = self.blocks[0]
        self._cur = 0
        b = self.block
        self._off_scores, self._off_flags, self._off_stats, self.nbytes = b._off_scores, b._off_flags, b._off_stats, b.nbytes

    def __del__(self):  # pragma: no cover
        try:
            for b in self.blocks:
                b.free()
        except Exception:
            pass

    # ---- the current block's views / addresses ----------------------------------------------------------------
    meta = property(lambda self: self.block.meta)
    scores = property(lambda self: self.block.scores)
    flags = property(lambda self: self.block.flags)
    stats = property(lambda self: self.block.stats)
    desc = property(lambda self: self.block.desc)
    h_seq = property(lambda self: self.block.h_seq)
    h_seq2 = property(lambda self: self.block.h_seq2)
    d_meta = property(lambda self: self.block.d_meta)
    d_scores = property(lambda self: self.block.d_scores)
    d_flags = property(lambda self: self.block.d_flags)
    h_stats_dst = property(lambda self: self.block.h_stats_dst)

    def flip(self) -> ResultBlock:
        """Make the OTHER block the current one for the report about to be enqueued (settling whatever its previous
        report -- two reports ago -- left behind) and return it."""
        nxt = self.blocks[1 - self._cur]
        if nxt._live is not None:
            nxt.settle()
        self._cur = 1 - self._cur
        self.block = nxt
        return nxt

    def attach(self, live) -> None:
        self.block.attach(live)

    def mark_live(self, seq: int) -> None:
        self.block.mark_live(seq)

    def settle(self) -> None:
        """Both blocks: nothing of this workspace is in flight or lazily referenced afterwards."""
        for b in self.blocks:
            if b._live is not None:
                b.settle()

    def host_block(self) -> np.ndarray:
        return self.block.host_block()

    def host_head(self) -> np.ndarray:
        return self.block.host_head()

    def host_head_bytes(self) -> bytes:
        return self.block.host_head_bytes()

    def host_stats(self, rows: int) -> np.ndarray:
        return self.block.host_stats(rows)

    # ---- kernel attribution (off unless a ReportGenerator asks: nothing is allocated before) -------------------
    _attr_buf = None      # device: the records of the last attribution of this workspace's table
    _attr_scratch = None  # device: column minima for the stateless operator
    _attr_last = None     # the Attribution whose kernel may still be reading the table / writing _attr_buf

    def attr_buffers(self, n_ranks: int, top_n: int, scratch: bool):
        """``(records buffer, scratch or None)`` for an attribution of ``n_ranks`` ranks (cold: allocated once per shape)."""
        words = _native.attr_words(n_ranks, top_n)
        dev = self._backend.device
        if self._attr_buf is None or self._attr_buf.numel() < words:
            with torch.cuda.stream(self._backend.stream):  # (allocated, written and read under the backend's stream)
                self._attr_buf = torch.empty(max(words, 64), dtype=torch.int32, device=dev)
        if scratch and self._attr_scratch is None:
            with torch.cuda.stream(self._backend.stream):
                self._attr_scratch = torch.empty(max(33 * self.K, 64), dtype=torch.float32, device=dev)
        return self._attr_buf, (self._attr_scratch if scratch else None)

    def attr_settle(self) -> None:
        """Before anything rewrites this workspace's table: the last attribution's kernel has run and its records are on the
        host (a ``Report`` still alive keeps them; an unread one costs this one small copy)."""
        last, self._attr_last = self._attr_last, None
        if last is not None:
            last.records()

    # ---- row families: tail, onset, period, episode scores (off unless a ReportGenerator asks: nothing is allocated before) ----
    _family_state = None  # family name -> _FamilyBuffers, once that family has run on this workspace

    def family_buffers(self, fam: RowFamily, group_words: int = 0):
        """``(send, table, scores, scratch)`` of one row family (cold: allocated on first use): ONE buffer holds the gathered
        table ``[R][P * (K+S)]`` and then the scores ``[R][1 + S]`` (one copy-out); ``send`` are this process' rows
        ``[local_ranks][P * (K+S)]`` (the table's own rows without an exchange); ``scratch`` takes the column minima.
        ``group_words`` (``_native.rowfam_group_words``: only the score step per peer group passes it): the buffer is ``table
        | pad to 16 bytes | column records | scores`` instead, and ``scores`` is what follows the pad.  It grows -- behind
        ``family_settle``, the table's contents carried over -- when there are more groups than before
        (``peer_groups="auto"``)."""
        if self._family_state is None:
            self._family_state = {}
        st = self._family_state.get(fam.name)
        KS, R, P = self.K + self.S, self.R, fam.planes
        head = (R * P * KS + 3) & ~3 if group_words else R * P * KS
        if st is None:
            st = self._family_state[fam.name] = _FamilyBuffers()
            dev = self._backend.device
            with torch.cuda.stream(self._backend.stream):  # (allocated, written and read under the backend's stream)
                st.buf = torch.empty(max(R * P * KS + R * (1 + self.S), head + group_words, 64), dtype=torch.float32, device=dev)
                st.table = st.buf[: R * P * KS].view(R, P * KS)
                st.send = (st.table if R == self.local_ranks
                           else torch.empty((self.local_ranks, P * KS), dtype=torch.float32, device=dev))
                st.scratch = torch.empty(max(33 * KS, 64), dtype=torch.float32, device=dev)
            st.last = None  # the RowScores whose kernels may still be reading the table / writing the buffers
        elif st.buf.numel() < head + group_words:  # cold: the first grouped step, or more groups than before
            self.family_settle(fam)
            with torch.cuda.stream(self._backend.stream):
                buf = torch.empty(head + group_words, dtype=torch.float32, device=self._backend.device)
                buf[: R * P * KS].copy_(st.buf[: R * P * KS])  # (this report's gathered table is in there already)
            table = buf[: R * P * KS].view(R, P * KS)
            if st.send is st.table:
                st.send = table
            st.buf, st.table = buf, table
        return st.send, st.table, st.buf[head:], st.scratch

    def family_settle(self, fam: RowFamily) -> None:
        """Before anything rewrites this workspace's table or that family's buffers: the family's last step's kernels have
        run and their results are on the host (a ``Report`` still alive keeps them; an unread one costs this one copy)."""
        st = self._family_state.get(fam.name) if self._family_state else None
        if st is not None and st.last is not None:
            last, st.last = st.last, None
            last.records()

    # (the families by name, as the backend and the rings have them: one-line delegations)
    def tail_buffers(self):
        return self.family_buffers(TAIL)

    def tail_settle(self) -> None:
        self.family_settle(TAIL)

    def onset_buffers(self):
        return self.family_buffers(ONSET)

    def onset_settle(self) -> None:
        self.family_settle(ONSET)

    def period_buffers(self):
        return self.family_buffers(PERIOD)

    def period_settle(self) -> None:
        self.family_settle(PERIOD)

    def episode_buffers(self):
        return self.family_buffers(EPISODE)

    def episode_settle(self) -> None:
        self.family_settle(EPISODE)

    def settle_readers(self) -> None:
        """Before a report rewrites this workspace's table: whatever follow-up kernel of the previous report may still be
        reading it -- attribution, tails, robust scores, onsets, periods, episodes -- has run and delivered; and so has the
        score history's step, which read the result block and wrote the records buffer."""
        if self._attr_last is not None:
            self.attr_settle()
        if self._family_state:
            self.family_settle(TAIL)
        if self._table_state:
            for fam in SLOTS:
                self.table_settle(fam)
        if self._family_state:
            for fam in FAMILIES[1:]:
                self.family_settle(fam)
        if self._history_last is not None:
            self.history_settle()
        if self._trend_last is not None:
            self.trend_settle()
        if self._peer_history_last is not None:
            self.peer_history_settle()
        if self._peer_trend_last is not None:
            self.peer_trend_settle()
        if self._slack_last is not None:
            self.slack_settle()
        if self._work_last is not None:
            self.work_settle()

    # ---- work groups (off unless a ReportGenerator asks: nothing is allocated before) -----------------------------
    _work_buf = None   # device: the block of the last work-group step on this workspace's table
    _work_last = None  # the Work whose kernels may still be reading the table / writing _work_buf

    def work_buffers(self):
        """The block of a work-group step over this workspace's table (cold: allocated once)."""
        if self._work_buf is None:
            with torch.cuda.stream(self._backend.stream):  # (allocated, written and read under the backend's stream)
                self._work_buf = torch.empty(max(_native.work_words(self.R, self.K, self.S), 64), dtype=torch.int32,
                                             device=self._backend.device)
        return self._work_buf

    def work_settle(self) -> None:
        """Before anything rewrites this workspace's table or the block: the last work-group step's kernels have run and its
        records are on the host (a ``Report`` still alive keeps them; an unread one costs this one small copy)."""
        last, self._work_last = self._work_last, None
        if last is not None:
            last.records()

    # ---- slack scores (off unless a ReportGenerator asks: nothing is allocated before) ----------------------------
    _slack_state = None  # (send, table, out) once a slack step has run on this workspace
    _slack_last = None   # the Slack whose kernels may still be reading the tables / writing the records

    def slack_buffers(self, group_words: int = 0):
        """``(send [local_ranks, 2 * 64] f32, table [R, 2 * 64] f32, out)`` of the slack step (cold: allocated on first
        use); ``send`` is the table itself when nothing is exchanged; ``out`` takes ``_native.slack_words(R)`` words, or
        ``group_words`` (``_native.slack_group_words``: the step per peer group) where that is more -- a report runs one of the
        two steps.  Only the per-group step passes ``group_words``, behind ``slack_settle``."""
        if self._slack_state is None:
            dev, W = self._backend.device, 2 * _native.SLACK_COLS
            with torch.cuda.stream(self._backend.stream):  # (allocated, written and read under the backend's stream)
                table = torch.empty((self.R, W), dtype=torch.float32, device=dev)
                send = table if self.R == self.local_ranks else torch.empty((self.local_ranks, W), dtype=torch.float32, device=dev)
                out = torch.empty(max(_native.slack_words(self.R), group_words), dtype=torch.int32, device=dev)
            self._slack_state = (send, table, out)
        elif self._slack_state[2].numel() < group_words:  # cold: more groups than before (peer_groups="auto")
            self.slack_settle()
            send, table, _ = self._slack_state
            with torch.cuda.stream(self._backend.stream):
                out = torch.empty(group_words, dtype=torch.int32, device=self._backend.device)
            self._slack_state = (send, table, out)
        return self._slack_state

    def slack_settle(self) -> None:
        """Before anything rewrites the slack step's buffers or this workspace's table: the last step's kernels have run and
        their records are on the host (a ``Report`` still alive keeps them; an unread one costs this one small copy)."""
        last, self._slack_last = self._slack_last, None
        if last is not None:
            last.records()

    # ---- table families: robust, peer, pace and node scores (off unless a ReportGenerator asks: nothing is allocated before) ----
    _table_state = None  # slot name -> _TableBuffers, once a family of that slot has run on this workspace

    def table_buffers(self, fam: TableFamily, n_ranks: int, G: int = 0):
        """The records buffer of ``fam``'s slot for ``n_ranks`` ranks in ``G`` groups (cold: allocated once per shape)."""
        words = fam.n_words(G, n_ranks, self.K, self.S)
        if self._table_state is None:
            self._table_state = {}
        st = self._table_state.get(fam.slot)
        if st is None:
            st = self._table_state[fam.slot] = _TableBuffers()
            st.buf = st.last = None  # last: the TableScores whose kernels may still be reading the table / writing buf
        if st.buf is None or st.buf.numel() < words:
            with torch.cuda.stream(self._backend.stream):  # (allocated, written and read under the backend's stream)
                st.buf = torch.empty(max(words, 64), dtype=torch.int32, device=self._backend.device)
        return st.buf

    def table_settle(self, fam: TableFamily) -> None:
        """Before anything rewrites this workspace's table or that slot's buffer: the slot's last step's kernels have run and
        their results are on the host (a ``Report`` still alive keeps them; an unread one costs this one small copy)."""
        st = self._table_state.get(fam.slot) if self._table_state else None
        if st is not None and st.last is not None:
            last, st.last = st.last, None
            last.records()

    # (the slots by name, as the cost tools and the tests have them: one-line delegations)
    def robust_buffers(self, n_ranks: int):
        return self.table_buffers(ROBUST, n_ranks)

    def robust_settle(self) -> None:
        self.table_settle(ROBUST)

    def peer_buffers(self, G: int, n_ranks: int):
        return self.table_buffers(PEER, n_ranks, G)

    def peer_settle(self) -> None:
        self.table_settle(PEER)

    def pace_buffers(self, n_ranks: int, G: int = 0):
        return self.table_buffers(PACE_GROUP if G else PACE, n_ranks, G)

    def pace_settle(self) -> None:
        self.table_settle(PACE)

    def node_buffers(self, G: int, n_ranks: int):
        return self.table_buffers(NODE, n_ranks, G)

    def node_settle(self) -> None:
        self.table_settle(NODE)

    # ---- score history (off unless a ReportGenerator asks: nothing is allocated before) ---------------------------
    _history_buf = None  # device: the records of the last history step on this workspace's result blocks
    _history_last = None  # the History whose kernel may still be reading a result block / writing _history_buf

    def history_buffers(self, n_ranks: int):
        """The records buffer for a history step over ``n_ranks`` ranks (cold: allocated once per shape)."""
        words = _native.history_words(n_ranks, self.S)
        if self._history_buf is None or self._history_buf.numel() < words:
            with torch.cuda.stream(self._backend.stream):  # (allocated, written and read under the backend's stream)
                self._history_buf = torch.empty(max(words, 64), dtype=torch.int32, device=self._backend.device)
        return self._history_buf

    def history_settle(self) -> None:
        """Before anything rewrites this workspace's result blocks or the records buffer: the last history step's kernel has
        run and its records are on the host (a ``Report`` still alive keeps them; an unread one costs this one small
        copy)."""
        last, self._history_last = self._history_last, None
        if last is not None:
            last.records()

    # ---- score trends (off unless a ReportGenerator asks: nothing is allocated before) ----------------------------
    _trend_buf = None   # device: the records of the last trend step issued through this workspace
    _trend_last = None  # the Trend whose kernel may still be writing _trend_buf

    def trend_buffers(self, n_ranks: int):
        """The records buffer for a trend step over ``n_ranks`` ranks (cold: allocated once per shape)."""
        words = _native.trend_words(n_ranks, self.S)
        if self._trend_buf is None or self._trend_buf.numel() < words:
            with torch.cuda.stream(self._backend.stream):  # (allocated, written and read under the backend's stream)
                self._trend_buf = torch.empty(max(words, 64), dtype=torch.int32, device=self._backend.device)
        return self._trend_buf

    def trend_settle(self) -> None:
        """Before anything rewrites the trend records buffer: the last trend step's kernel has run and its records are on
        the host (a ``Report`` still alive keeps them; an unread one costs this one small copy)."""
        last, self._trend_last = self._trend_last, None
        if last is not None:
            last.records()

    # ---- peer-score history and trends (off unless a ReportGenerator asks: nothing is allocated before) ------------
    _peer_history_buf = None   # device: the records of the last peer-history step issued through this workspace
    _peer_history_last = None  # the History whose kernel may still be reading the peer slot / writing _peer_history_buf
    _peer_trend_buf = None     # device: the records of the last peer-trend step issued through this workspace
    _peer_trend_last = None    # the Trend whose kernel may still be writing _peer_trend_buf

    def _records_buffer(self, attr: str, words: int):
        buf = getattr(self, attr)
        if buf is None or buf.numel() < words:
            with torch.cuda.stream(self._backend.stream):  # (allocated, written and read under the backend's stream)
                buf = torch.empty(max(words, 64), dtype=torch.int32, device=self._backend.device)
            setattr(self, attr, buf)
        return buf

    def peer_history_buffers(self, n_ranks: int):
        """The records buffer for a peer-history step over ``n_ranks`` ranks (cold: allocated once per shape)."""
        return self._records_buffer("_peer_history_buf", _native.peer_history_words(n_ranks, self.S))

    def peer_history_settle(self) -> None:
        """Before anything rewrites the peer slot's block or the records buffer: the last peer-history step's kernel has run
        and its records are on the host (a ``Report`` still alive keeps them; an unread one costs this one small copy)."""
        last, self._peer_history_last = self._peer_history_last, None
        if last is not None:
            last.records()

    def peer_trend_buffers(self, n_ranks: int):
        """The records buffer for a peer-trend step over ``n_ranks`` ranks (cold: allocated once per shape)."""
        return self._records_buffer("_peer_trend_buf", _native.peer_trend_words(n_ranks, self.S))

    def peer_trend_settle(self) -> None:
        """Before anything rewrites the peer-trend records buffer: the last step's kernel has run and its records are on the
        host (a ``Report`` still alive keeps them; an unread one costs this one small copy)."""
        last, self._peer_trend_last = self._peer_trend_last, None
        if last is not None:
            last.records()

    def set_send_row(self, lr: int, row: np.ndarray) -> None:
        """Host-packed exchange row (dict-input path)."""
        self.send[lr].copy_(torch.from_numpy(row), non_blocking=False)
        self.send_initialised = True


def _stream_priority() -> int:
    """Priority of the detector's own streams (``NVRX_STREAM_PRIORITY=high|normal``, default high): a report that runs BESIDE
    the training stream -- asynchronous reports, synchronous ones that cannot be re-homed -- competes with GEMMs for compute
    units; on a high-priority queue its few workgroups are dispatched ahead of the GEMM's next ones instead of behind them
    (nothing running is preempted).  Same-box A/B, three alternating rounds of config #4: a report every step costs the step
    1.15 / 1.15 / 0.80 % at normal priority, 0.96 / 0.83 / 0.77 % at high (asynchronous); 3.43 / 3.10 / 2.93 against
    3.01 / 3.00 / 2.91 % (synchronous); no effect on an idle GPU (profiles/r04p_stream_priority.txt).

    That is the default of a SINGLE-process job only.  In a multi-rank job the detector's stream also carries the report's
    RCCL all-gather, beside the job's own collectives on other streams and communicators; which of two communicators' kernels
    is dispatched first is better left to the order they were enqueued in until a run across real GPUs says otherwise, so the
    default there stays normal (``NVRX_STREAM_PRIORITY=high`` asks for it by name)."""
    want = os.environ.get("NVRX_STREAM_PRIORITY", "").strip().lower()
    if not want:
        from . import ktrace as _ktrace  # (the launcher's job size: WORLD_SIZE, else srun's / mpirun's / PMI's)

        want = "normal" if _ktrace._job_size()[0] > 1 else "high"  # (the library applies the same rule to the resident scorer's stream)
    return 0 if want in ("normal", "0", "off") else -1


class HipBackend:
    """MI355X engine: owns the side stream the report runs on and the per-shape workspaces."""

    name = "hip"

    def __init__(self, device: Optional[int] = None):
        self.lib = _native.load()
        if not torch.cuda.is_available():
            raise RuntimeError(_NO_DEVICE)
        index = torch.cuda.current_device() if device is None else int(device)
        self.device = torch.device("cuda", index)
        # the report pipeline runs on its own stream so it never serialises with the training stream
        self.stream = torch.cuda.Stream(device=self.device, priority=_stream_priority())
        self._workspaces = {}
        self._retired = []
        self._thr = (ctypes.c_double * 4)(*DEFAULT_THRESHOLDS)
        self._thr_src = DEFAULT_THRESHOLDS
        self._stream_handle = self.stream.cuda_stream

    @property
    def stream_handle(self) -> int:
        return self._stream_handle

    def stream_context(self):
        return torch.cuda.stream(self.stream)

    def current_stream_handle(self) -> int:
        """hipStream_t of the stream user code is currently launching on (for region timing)."""
        return _raw_current_stream(self.device.index)

    def workspace(self, R: int, K: int, S: int, local_ranks: int = 1, stats_rows: int = 0) -> Workspace:
        key = (R, K, S, local_ranks, stats_rows)
        ws = self._workspaces.get(key)
        if ws is None:
            if len(self._workspaces) > 8:  # shapes only change when new names appear
                self._workspaces.clear()
            with torch.cuda.device(self.device):
                ws = Workspace(self, R, K, S, local_ranks, stats_rows)
                # the buffers were zero-filled on torch's current stream; the report runs on ours
                torch.cuda.current_stream().synchronize()
            self._workspaces[key] = ws
        return ws

    def make_rings(self, local_ranks: int, rows_per_rank: int, ring_cap: int) -> "HipRings":
        return HipRings(self, local_ranks, rows_per_rank, ring_cap)

    def send_init(self, ws: Workspace) -> None:
        _native.check(self.lib.nvrx_send_init(ws.send.data_ptr(), ws.local_ranks, ws.K, ws.S, self.stream_handle))
        ws.send_initialised = True

    def score(self, ws: Workspace, table: torch.Tensor, do_indiv: bool, do_rel: bool,
              thresholds: Sequence[float] = DEFAULT_THRESHOLDS, wait: bool = True,
              stats_rows: Optional[int] = None) -> None:
        """Score kernel, then spin on the completion word it publishes into the pinned result block
        (two C calls, no torch dispatch, no D2H copy, no stream sync); on return
        ``ws.scores/flags/meta/stats`` hold this report's values."""
        if thresholds is not self._thr_src:
            for i in range(4):
                self._thr[i] = float(thresholds[i])
            self._thr_src = thresholds
        lib = self.lib
        blk = ws.flip()  # this report's result block; the previous report's block stays readable for one more report
        nrows = ws.stats_rows if stats_rows is None else min(stats_rows, ws.stats_rows)
        table_ptr = ws.table_ptr if table is ws.table else (ws.send_ptr if table is ws.send else table.data_ptr())
        ws.seq = (ws.seq % 0x7FFFFFFF) + 1  # one sequence for both report routes and both blocks
        rc = lib.nvrx_score(table_ptr, ws.R, ws.K, ws.S, int(do_indiv), int(do_rel), self._thr,
                            blk.d_scores, blk.d_flags, blk.d_meta, ws.d_counter, ws.seq,
                            ws.d_stats, blk.h_stats_dst, nrows, self._stream_handle)
        if rc < 0:
            _native.check(rc)
        if wait:
            timeout = report_timeout_s()
            rc = lib.nvrx_poll_u32(blk.h_seq, ws.seq, timeout if timeout > 0 else 1e30)
            if rc < 0:
                self.retire_workspace(ws)
                _native.check(rc)

    def wait_seq(self, ws: Optional[Workspace], seq: int, stats: bool = False, block: Optional[ResultBlock] = None) -> None:
        """Block until the report that was enqueued with sequence number ``seq`` has published its results into
        ``block`` (default: the workspace's current one); ``stats=True``: its statistics rows, which a resident score
        kernel forwards after the scores."""
        blk = block if block is not None else ws.block
        timeout = report_timeout_s()
        rc = self.lib.nvrx_poll_u32(blk.h_seq2 if stats else blk.h_seq, seq, timeout if timeout > 0 else 1e30)
        if rc < 0:
            if ws is None:
                ws = next((w for w in self._workspaces.values() if blk in w.blocks), None)
            if ws is not None:
                self.retire_workspace(ws)
            _native.check(rc)

    def attribute(self, ws: Workspace, table: torch.Tensor, top_n: int, do_indiv: bool, do_rel: bool,
                  first_rank: int = 0, n_ranks: Optional[int] = None) -> Attribution:
        """Kernel attribution of ``table`` ([R, L], the table ``score`` was given) for ranks ``[first_rank, first_rank +
        n_ranks)``: ``nvrx_attribute`` enqueued on the backend's stream behind the score kernel.  Nothing is waited for."""
        n_ranks = ws.R - first_rank if n_ranks is None else n_ranks
        ws.attr_settle()
        buf, scratch = ws.attr_buffers(n_ranks, top_n, bool(do_rel))
        table_ptr = ws.table_ptr if table is ws.table else (ws.send_ptr if table is ws.send else table.data_ptr())
        rc = self.lib.nvrx_attribute(table_ptr, ws.R, ws.K, ws.S, first_rank, n_ranks, top_n, int(do_indiv), int(do_rel),
                                     scratch.data_ptr() if scratch is not None else None, buf.data_ptr(), self._stream_handle)
        if rc < 0:
            _native.check(rc)
        out = ws._attr_last = Attribution(self, buf, first_rank, n_ranks, top_n)
        return out

    def attribution_copy_out(self, attr: Attribution) -> np.ndarray:
        """The one wait of an attribution: a D2H of its records on the backend's stream, behind its kernel."""
        host = np.empty((attr.n_ranks, 2, 1 + attr.top_n, 4), dtype=np.uint32)
        _native.check(self.lib.nvrx_d2h_sync(host.ctypes.data, attr.d_ptr, host.nbytes, self._stream_handle))
        return host

    def _family_score(self, fam: RowFamily, ws: Workspace, planes: torch.Tensor, table: torch.Tensor, first_rank: int,
                      n_ranks: Optional[int], params: tuple = ()) -> RowScores:
        """Relative scores of one row family for ranks ``[first_rank, first_rank + n_ranks)`` from its gathered table
        ``planes`` ([R, P * (K+S)], ``Rings.<family>_local``'s) and the weights in ``table`` ([R, L], the table ``score`` was
        given): ``nvrx_<family>_score`` enqueued on the backend's stream.  Nothing is waited for."""
        n_ranks = ws.R - first_rank if n_ranks is None else n_ranks
        _, fam_table, scores, scratch = ws.family_buffers(fam)
        assert planes is fam_table or (planes.data_ptr() == fam_table.data_ptr())
        table_ptr = ws.table_ptr if table is ws.table else (ws.send_ptr if table is ws.send else table.data_ptr())
        rc = getattr(self.lib, fam.c_score)(fam_table.data_ptr(), table_ptr, ws.R, ws.K, ws.S, first_rank, n_ranks,
                                            scratch.data_ptr(), scores.data_ptr(), self._stream_handle)
        if rc < 0:
            _native.check(rc)
        st = ws._family_state[fam.name]
        out = st.last = RowScores(self, fam, st.buf, ws.R, ws.K, ws.S, first_rank, n_ranks, params)
        return out

    def _family_group_score(self, fam: RowFamily, ws: Workspace, planes: torch.Tensor, table: torch.Tensor, groups: PeerGroups,
                            first_rank: int, n_ranks: Optional[int], min_ranks: int, params: tuple = ()) -> RowGroupScores:
        """``_family_score`` per peer group: a column's reference is taken inside each rank's own group of the resolved
        ``groups``, a pair needing ``min_ranks`` present members (``nvrx_rowfam_group_score`` enqueued on the backend's
        stream, in the slot of the job-wide step).  Nothing is waited for."""
        n_ranks = ws.R - first_rank if n_ranks is None else n_ranks
        if groups.R != ws.R:
            raise ValueError(f"peer groups of {groups.R} ranks for a table of {ws.R}")
        _, before, _, _ = ws.family_buffers(fam)
        assert planes is before or (planes.data_ptr() == before.data_ptr())
        _, fam_table, out, _ = ws.family_buffers(fam, _native.rowfam_group_words(groups.G, ws.K, ws.S, n_ranks))
        table_ptr = ws.table_ptr if table is ws.table else (ws.send_ptr if table is ws.send else table.data_ptr())
        rc = self.lib.nvrx_rowfam_group_score(fam_table.data_ptr(), fam.planes, table_ptr, ws.R, ws.K, ws.S,
                                              groups.device(self).data_ptr(), groups.G, first_rank, n_ranks, int(min_ranks),
                                              out.data_ptr(), self._stream_handle)
        if rc < 0:
            _native.check(rc)
        st = ws._family_state[fam.name]
        handle = st.last = RowGroupScores(self, fam, st.buf, ws.R, ws.K, ws.S, groups.G, first_rank, n_ranks, int(min_ranks), params)
        return handle

    def family_group_copy_out(self, t: RowGroupScores):
        """The one wait of a report's row family per peer group: a D2H of its table, column records and scores on the
        backend's stream, behind the kernels."""
        KS, P = t.K + t.S, t.family.planes
        head = (t.R * P * KS + 3) & ~3
        n = head + _native.rowfam_group_words(t.G, t.K, t.S, t.n_ranks)
        host = np.empty(n, dtype=np.float32)
        _native.check(self.lib.nvrx_d2h_sync(host.ctypes.data, t.d_ptr, n * 4, self._stream_handle))
        shape = (t.R, KS) if P == 1 else (t.R, P, KS)
        planes = host[: t.R * P * KS].reshape(shape)[t.first_rank : t.first_rank + t.n_ranks].copy()
        cols = host[head : head + 4 * t.G * KS].view(np.uint32).reshape(t.G, KS, 4).copy()
        return planes, host[head + 4 * t.G * KS : n].reshape(t.n_ranks, 1 + t.S).copy(), cols

    def tail_group_score(self, ws, tails, table, groups, first_rank: int = 0, n_ranks: Optional[int] = None, min_ranks: int = 2,
                         q_ppm: int = 0) -> RowGroupScores:
        return self._family_group_score(TAIL, ws, tails, table, groups, first_rank, n_ranks, min_ranks, (q_ppm,))

    def onset_group_score(self, ws, onsets, table, groups, first_rank: int = 0, n_ranks: Optional[int] = None,
                          min_ranks: int = 2) -> RowGroupScores:
        return self._family_group_score(ONSET, ws, onsets, table, groups, first_rank, n_ranks, min_ranks)

    def period_group_score(self, ws, periods, table, groups, first_rank: int = 0, n_ranks: Optional[int] = None,
                           min_ranks: int = 2) -> RowGroupScores:
        return self._family_group_score(PERIOD, ws, periods, table, groups, first_rank, n_ranks, min_ranks)

    def episode_group_score(self, ws, episodes, table, groups, first_rank: int = 0, n_ranks: Optional[int] = None,
                            min_ranks: int = 2) -> RowGroupScores:
        return self._family_group_score(EPISODE, ws, episodes, table, groups, first_rank, n_ranks, min_ranks)

    def family_copy_out(self, t: RowScores):
        """The one wait of a report's row family: a D2H of its table and scores on the backend's stream, behind the kernels."""
        KS, P = t.K + t.S, t.family.planes
        n = t.R * P * KS + t.n_ranks * (1 + t.S)
        host = np.empty(max(n, 1), dtype=np.float32)
        if n:
            _native.check(self.lib.nvrx_d2h_sync(host.ctypes.data, t.d_ptr, n * 4, self._stream_handle))
        shape = (t.R, KS) if P == 1 else (t.R, P, KS)
        planes = host[: t.R * P * KS].reshape(shape)[t.first_rank : t.first_rank + t.n_ranks].copy()
        return planes, host[t.R * P * KS : n].reshape(t.n_ranks, 1 + t.S).copy()

    def tails_copy_out(self, t: RowScores):
        return self.family_copy_out(t)

    def onsets_copy_out(self, t: RowScores):
        return self.family_copy_out(t)

    def periods_copy_out(self, t: RowScores):
        return self.family_copy_out(t)

    def episodes_copy_out(self, t: RowScores):
        return self.family_copy_out(t)

    def tail_score(self, ws, tails, table, first_rank: int = 0, n_ranks: Optional[int] = None, q_ppm: int = 0) -> RowScores:
        return self._family_score(TAIL, ws, tails, table, first_rank, n_ranks, (q_ppm,))

    def onset_score(self, ws, onsets, table, first_rank: int = 0, n_ranks: Optional[int] = None) -> RowScores:
        return self._family_score(ONSET, ws, onsets, table, first_rank, n_ranks)

    def period_score(self, ws, periods, table, first_rank: int = 0, n_ranks: Optional[int] = None) -> RowScores:
        return self._family_score(PERIOD, ws, periods, table, first_rank, n_ranks)

    def episode_score(self, ws, episodes, table, first_rank: int = 0, n_ranks: Optional[int] = None) -> RowScores:
        return self._family_score(EPISODE, ws, episodes, table, first_rank, n_ranks)

    def _row_op(self, fam: RowFamily, samples: torch.Tensor, counts: torch.Tensor, param: int,
                starts: Optional[torch.Tensor]) -> torch.Tensor:
        """A family's stateless operator on caller tensors ([rows, stride] f32, [rows] u32/i32 counts and ring starts) ->
        [rows, 4] int32 records, the last three words f32 bit patterns (``nvrx_row_<family>``, include/nvrx_straggler.h)."""
        rows, stride = samples.shape
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(self.stream):
            out = torch.empty((max(rows, 1), 4), dtype=torch.int32, device=samples.device)
            _native.check(getattr(self.lib, fam.c_row)(samples.data_ptr(), counts.data_ptr(),
                                                       starts.data_ptr() if starts is not None else None, rows, stride,
                                                       int(param), out.data_ptr(), self.stream_handle))
        self.stream.synchronize()
        return out[:rows]

    def row_onset(self, samples, counts, min_seg_ppm: int, starts=None) -> torch.Tensor:
        """Records ``{ago, before, after, strength}``."""
        return self._row_op(ONSET, samples, counts, min_seg_ppm, starts)

    def row_period(self, samples, counts, max_period: int, starts=None) -> torch.Tensor:
        """Records ``{period | ago << 16, peak, rest, strength}``."""
        return self._row_op(PERIOD, samples, counts, max_period, starts)

    def row_episode(self, samples, counts, min_len_ppm: int, starts=None) -> torch.Tensor:
        """Records ``{ago | length << 16, inside, outside, strength}``."""
        return self._row_op(EPISODE, samples, counts, min_len_ppm, starts)

    def _table_step(self, fam: TableFamily, ws: Workspace, entry, head: tuple, tail: tuple, groups: Optional[PeerGroups],
                    first_rank: int, n_ranks: Optional[int], params: tuple) -> TableScores:
        """What both routes of a table family share: the slot settled, its buffer, ``entry(*head, [d_groups, G, [max_size]],
        rank range and parameters in the family's order, d_out, *tail)``, and the handle noted in the slot."""
        n_ranks = ws.R - first_rank if n_ranks is None else n_ranks
        G, lead = 0, ()
        if fam.groups:
            if groups.R != ws.R:
                raise ValueError(f"{fam.groups} groups resolved for {groups.R} ranks, the table has {ws.R}")
            G = groups.G
            lead = (groups.device(self).data_ptr(), G, groups.max_size) if fam.max_size else (groups.device(self).data_ptr(), G)
        ws.table_settle(fam)  # (the records buffer is about to be rewritten)
        buf = ws.table_buffers(fam, n_ranks, G)
        rc = entry(*head, *lead, *fam.rank_args(first_rank, n_ranks, params), buf.data_ptr(), *tail)
        if rc < 0:
            _native.check(rc)
        out = ws._table_state[fam.slot].last = TableScores(self, fam, buf, G, ws.K, ws.S, first_rank, n_ranks, params)
        return out

    def _table_score(self, fam: TableFamily, ws: Workspace, table: torch.Tensor, groups: Optional[PeerGroups], first_rank: int,
                     n_ranks: Optional[int], params: tuple) -> TableScores:
        """One table family's scores of ``table`` ([R, L], the table ``score`` was given) for ranks ``[first_rank, first_rank
        + n_ranks)``, with the ranks of ``groups`` where the family takes them: ``nvrx_<family>_score`` enqueued on the
        backend's stream behind the score kernel.  Nothing is waited for."""
        table_ptr = ws.table_ptr if table is ws.table else (ws.send_ptr if table is ws.send else table.data_ptr())
        return self._table_step(fam, ws, getattr(self.lib, fam.c_score), (table_ptr, ws.R, ws.K, ws.S), (self._stream_handle,),
                                groups, first_rank, n_ranks, params)

    def table_copy_out(self, t: TableScores):
        """The one wait of a report's table family: a D2H of its block on the backend's stream, behind the kernels."""
        n = t.family.n_words(t.G, t.n_ranks, t.K, t.S)
        host = np.empty(n, dtype=np.uint32)
        _native.check(self.lib.nvrx_d2h_sync(host.ctypes.data, t.d_ptr, n * 4, self._stream_handle))
        return t.family.cut(host, t.G, t.n_ranks, t.K, t.S)

    # (the families by name, as reporting.py, the oracle backends and the tests have them: one-line delegations)
    def robust_score(self, ws: Workspace, table: torch.Tensor, first_rank: int = 0, n_ranks: Optional[int] = None,
                     min_ranks: int = 4, floor_rel: float = 0.02) -> TableScores:
        return self._table_score(ROBUST, ws, table, None, first_rank, n_ranks, (min_ranks, floor_rel))

    def peer_score(self, ws: Workspace, table: torch.Tensor, groups: PeerGroups, first_rank: int = 0,
                   n_ranks: Optional[int] = None, min_ranks: int = 2) -> TableScores:
        return self._table_score(PEER, ws, table, groups, first_rank, n_ranks, (min_ranks,))

    def pace_score(self, ws: Workspace, table: torch.Tensor, first_rank: int = 0, n_ranks: Optional[int] = None,
                   min_ranks: int = 4) -> TableScores:
        return self._table_score(PACE, ws, table, None, first_rank, n_ranks, (min_ranks,))

    def pace_group_score(self, ws: Workspace, table: torch.Tensor, groups: PeerGroups, first_rank: int = 0,
                         n_ranks: Optional[int] = None, min_ranks: int = 4, min_peers: int = 2) -> TableScores:
        return self._table_score(PACE_GROUP, ws, table, groups, first_rank, n_ranks, (min_ranks, min_peers))

    def node_score(self, ws: Workspace, table: torch.Tensor, nodes: PeerGroups, first_rank: int = 0,
                   n_ranks: Optional[int] = None, min_members: int = 2, min_nodes: int = 3) -> TableScores:
        return self._table_score(NODE, ws, table, nodes, first_rank, n_ranks, (min_members, min_nodes))

    def robust_copy_out(self, t: TableScores):
        return self.table_copy_out(t)

    def peer_copy_out(self, t: TableScores):
        return self.table_copy_out(t)

    def pace_copy_out(self, t: TableScores):
        return self.table_copy_out(t)

    def pace_group_copy_out(self, t: TableScores):
        return self.table_copy_out(t)

    def node_copy_out(self, t: TableScores):
        return self.table_copy_out(t)

    def history_prepare(self, ws: Workspace, state: ScoreHistory, first_rank: int, n_ranks: int, thresholds):
        """What both routes of a history step share: the ring of ``state`` with room for this workspace's section ids (cold:
        allocated -- every word a NaN -- or grown on the backend's stream, the old entries copied by slicing: ids are never
        reassigned, so old columns keep their history), the records buffer, and the thresholds as the library takes them."""
        state.begin(first_rank, n_ranks)
        if state.hist is None or ws.S > state.S_cap:
            cap = ScoreHistory.capacity(ws.S)
            with torch.cuda.stream(self.stream):  # (allocated, written and read under the backend's stream)
                ring = torch.full((n_ranks, 2, 1 + cap, 4 * state.stride), 0xFF, dtype=torch.uint8,
                                  device=self.device).view(torch.float32)
                if state.hist is not None:
                    ring[:, :, : 1 + state.S_cap] = state.hist
            state.hist, state.S_cap = ring, cap
        ws.history_settle()
        thr = tuple(float(t) for t in thresholds)
        if len(thr) != 4:
            raise ValueError(f"a score history takes four thresholds, got {thresholds!r}")
        return ws.history_buffers(n_ranks), (ctypes.c_double * 4)(*thr)

    def score_history(self, ws: Workspace, state: ScoreHistory, first_rank: int = 0, n_ranks: Optional[int] = None,
                      thresholds: Sequence[float] = DEFAULT_THRESHOLDS) -> History:
        """Append the scores ``score`` just left in ``ws``'s current result block to ``state``'s ring, for ranks
        ``[first_rank, first_rank + n_ranks)``: ``nvrx_score_history`` enqueued on the backend's stream behind the score
        kernel.  Nothing is waited for."""
        n_ranks = ws.R - first_rank if n_ranks is None else n_ranks
        buf, c_thr = self.history_prepare(ws, state, first_rank, n_ranks, thresholds)
        rc = self.lib.nvrx_score_history(ws.d_scores, ws.R, ws.S, first_rank, n_ranks, state.hist.data_ptr(), state.S_cap,
                                         state.depth, state.n_before, c_thr, buf.data_ptr(), self._stream_handle)
        if rc < 0:
            _native.check(rc)
        state.n_before += 1
        out = ws._history_last = History(self, buf, ws.S, first_rank, n_ranks)
        return out

    def history_copy_out(self, h: History) -> np.ndarray:
        """The one wait of a report's score history: a D2H of the records on the backend's stream, behind the kernel."""
        host = np.empty((h.n_ranks, h.fams, 1 + h.S, _native.HISTORY_RECORD_WORDS), dtype=np.uint32)
        _native.check(self.lib.nvrx_d2h_sync(host.ctypes.data, h.d_ptr, host.nbytes, self._stream_handle))
        return host

    def score_trend(self, ws: Workspace, state: ScoreHistory) -> Trend:
        """The trends of ``state``'s ring as the history step just issued on ``ws`` leaves it (``score_history``;
        ``state.n_before`` counts that report): ``nvrx_score_trend`` enqueued on the backend's stream behind that step.
        Nothing is waited for."""
        ws.trend_settle()
        n_ranks = state.ranks[1]
        buf = ws.trend_buffers(n_ranks)
        rc = self.lib.nvrx_score_trend(state.hist.data_ptr(), n_ranks, ws.S, state.S_cap, state.depth, state.n_before,
                                       buf.data_ptr(), self._stream_handle)
        if rc < 0:
            _native.check(rc)
        out = ws._trend_last = Trend(self, buf, ws.S, n_ranks)
        return out

    def trend_copy_out(self, t: Trend) -> np.ndarray:
        """The one wait of a report's score trends: a D2H of the records on the backend's stream, behind the kernel."""
        host = np.empty((t.n_ranks, t.fams, 1 + t.S, _native.TREND_RECORD_WORDS), dtype=np.uint32)
        _native.check(self.lib.nvrx_d2h_sync(host.ctypes.data, t.d_ptr, host.nbytes, self._stream_handle))
        return host

    def _peer_history_step(self, ws: Workspace, state: PeerHistory, peer: TableScores, thresholds, entry, head: tuple,
                           tail: tuple) -> History:
        """What both routes of a peer-history step share: the ring of ``state`` with room for this workspace's section ids
        (cold: allocated -- every word a NaN -- or grown on the backend's stream, the old entries copied by slicing), the
        records buffer settled, ``entry(*head, the rank part of ``peer``'s block, shape, ring, thresholds, d_out, *tail)`` and
        the handle noted in the workspace.  ``peer`` is the handle of the peer step just issued on ``ws``: its block sits in
        the workspace's peer slot, which nothing settles or rewrites between that step and this one."""
        first_rank, n_ranks = peer.first_rank, peer.n_ranks
        state.begin(first_rank, n_ranks)
        if state.hist is None or ws.S > state.S_cap:
            cap = ScoreHistory.capacity(ws.S)
            with torch.cuda.stream(self.stream):  # (allocated, written and read under the backend's stream)
                ring = torch.full((n_ranks, 1 + cap, 4 * state.stride), 0xFF, dtype=torch.uint8,
                                  device=self.device).view(torch.float32)
                if state.hist is not None:
                    ring[:, : 1 + state.S_cap] = state.hist
            state.hist, state.S_cap = ring, cap
        ws.peer_history_settle()
        thr = tuple(float(t) for t in thresholds)
        if len(thr) != 2:
            raise ValueError(f"a peer-score history takes two thresholds (gpu, section), got {thresholds!r}")
        buf = ws.peer_history_buffers(n_ranks)
        d_peer = peer.d_ptr + 16 * peer.G * (peer.K + peer.S)  # behind the G (K+S) column records of 16 bytes
        rc = entry(*head, d_peer, n_ranks, ws.S, state.hist.data_ptr(), state.S_cap, state.depth, state.n_before,
                   (ctypes.c_double * 2)(*thr), buf.data_ptr(), *tail)
        if rc < 0:
            _native.check(rc)
        state.n_before += 1
        out = ws._peer_history_last = History(self, buf, ws.S, first_rank, n_ranks, fams=1)
        return out

    def peer_history(self, ws: Workspace, state: PeerHistory, peer: TableScores,
                     thresholds: Sequence[float] = (0.75, 0.75)) -> History:
        """Append the peer scores ``peer_score`` just left in ``ws``'s peer slot (``peer``: that step's handle) to ``state``'s
        ring: ``nvrx_peer_history`` enqueued on the backend's stream directly behind that step.  Nothing is waited for."""
        return self._peer_history_step(ws, state, peer, thresholds, self.lib.nvrx_peer_history, (), (self._stream_handle,))

    def _peer_trend_step(self, ws: Workspace, state: PeerHistory, entry, head: tuple, tail: tuple) -> Trend:
        ws.peer_trend_settle()
        n_ranks = state.ranks[1]
        buf = ws.peer_trend_buffers(n_ranks)
        rc = entry(*head, state.hist.data_ptr(), n_ranks, ws.S, state.S_cap, state.depth, state.n_before, buf.data_ptr(), *tail)
        if rc < 0:
            _native.check(rc)
        out = ws._peer_trend_last = Trend(self, buf, ws.S, n_ranks, fams=1)
        return out

    def peer_trend(self, ws: Workspace, state: PeerHistory) -> Trend:
        """The trends of ``state``'s ring as the peer-history step just issued on ``ws`` leaves it (``state.n_before`` counts
        that report): ``nvrx_peer_trend`` enqueued on the backend's stream behind that step.  Nothing is waited for."""
        return self._peer_trend_step(ws, state, self.lib.nvrx_peer_trend, (), (self._stream_handle,))

    def _work_step(self, ws: Workspace, entry, head: tuple, tail: tuple, count_tol: float, max_unlike_ppm: int) -> Work:
        """What both routes of the work-group step share: the slot settled, its block, ``entry(*head, count_tol,
        max_unlike_ppm, d_out, *tail)``, and the handle noted in the workspace."""
        ws.work_settle()  # (the block is about to be rewritten)
        buf = ws.work_buffers()
        rc = entry(*head, float(count_tol), int(max_unlike_ppm), buf.data_ptr(), *tail)
        if rc < 0:
            _native.check(rc)
        out = ws._work_last = Work(self, buf, ws.R, ws.K, ws.S, float(count_tol), int(max_unlike_ppm))
        return out

    def work_groups(self, ws: Workspace, table: torch.Tensor, count_tol: float = 0.25, max_unlike_ppm: int = 100000) -> Work:
        """Which ranks of ``table`` ([R, L], the table ``score`` was given) do the same work: ``nvrx_work_groups`` enqueued on
        the backend's stream behind the score kernel.  All R ranks are computed.  Nothing is waited for."""
        table_ptr = ws.table_ptr if table is ws.table else (ws.send_ptr if table is ws.send else table.data_ptr())
        return self._work_step(ws, self.lib.nvrx_work_groups, (table_ptr, ws.R, ws.K, ws.S), (self._stream_handle,), count_tol,
                               max_unlike_ppm)

    def work_copy_out(self, w: Work):
        """The one wait of a report's work groups: a D2H of the rank records and the job record, which end the block, on the
        backend's stream, behind the kernels."""
        _, _, rank, job, words = _native.work_offsets(w.R, w.K, w.S)
        host = np.empty(words - rank, dtype=np.uint32)
        _native.check(self.lib.nvrx_d2h_sync(host.ctypes.data, w.d_ptr + 4 * rank, host.nbytes, self._stream_handle))
        return host[: job - rank].reshape(w.R, _native.WORK_RANK_WORDS).copy(), host[job - rank:].copy()

    def slack_score(self, ws: Workspace, slack_table: torch.Tensor, table: torch.Tensor, first_rank: int = 0,
                    n_ranks: Optional[int] = None, min_ranks: int = 4) -> Slack:
        """Slack scores from the gathered rows ``slack_table`` ([R, 2 * 64], ``HipRings.slack_local`` and the caller's
        all-gather) and ``table`` ([R, L], the table ``score`` was given; its kernel weights are the compute time):
        ``nvrx_slack_score`` enqueued on the backend's stream.  All R ranks are computed; the handle delivers ranks
        ``[first_rank, first_rank + n_ranks)``.  Nothing is waited for."""
        n_ranks = ws.R - first_rank if n_ranks is None else n_ranks
        if first_rank < 0 or n_ranks < 1 or first_rank + n_ranks > ws.R:
            raise ValueError(f"ranks [{first_rank}, {first_rank}+{n_ranks}) outside the table's {ws.R}")
        _, _, out = ws.slack_buffers()
        table_ptr = ws.table_ptr if table is ws.table else (ws.send_ptr if table is ws.send else table.data_ptr())
        rc = self.lib.nvrx_slack_score(slack_table.data_ptr(), table_ptr, ws.R, ws.K, ws.S, min(int(min_ranks), ws.R),
                                       out.data_ptr(), self._stream_handle)
        if rc < 0:
            _native.check(rc)
        handle = ws._slack_last = Slack(self, out, first_rank, n_ranks, min(int(min_ranks), ws.R))
        return handle

    def slack_copy_out(self, s: Slack):
        """The one wait of a report's slack scores: a D2H of the head and of the rank records up to the last rank the report
        covers, on the backend's stream, behind the kernels."""
        head, rw = _native.SLACK_HEAD_WORDS, _native.SLACK_RANK_WORDS
        n = head + rw * (s.first_rank + s.n_ranks)
        host = np.empty(n, dtype=np.uint32)
        _native.check(self.lib.nvrx_d2h_sync(host.ctypes.data, s.d_ptr, n * 4, self._stream_handle))
        return (host[:8].copy(), host[8:head].reshape(_native.SLACK_COLS, 4).copy(),
                host[head + rw * s.first_rank:].reshape(s.n_ranks, rw).copy())

    def slack_group_score(self, ws: Workspace, slack_table: torch.Tensor, table: torch.Tensor, groups: PeerGroups,
                          first_rank: int = 0, n_ranks: Optional[int] = None, min_ranks: int = 4,
                          min_peers: int = 2) -> SlackGroup:
        """Slack scores per peer group from the gathered rows ``slack_table`` and ``table``, as ``slack_score`` takes them,
        and the resolved ``groups``: ``nvrx_slack_group_score`` enqueued on the backend's stream, in the slot of the job-wide
        step.  All R ranks are computed; the handle delivers every group's record and pair records and the ranks
        ``[first_rank, first_rank + n_ranks)``.  Nothing is waited for."""
        n_ranks = ws.R - first_rank if n_ranks is None else n_ranks
        if first_rank < 0 or n_ranks < 1 or first_rank + n_ranks > ws.R:
            raise ValueError(f"ranks [{first_rank}, {first_rank}+{n_ranks}) outside the table's {ws.R}")
        if groups.R != ws.R:
            raise ValueError(f"peer groups of {groups.R} ranks for a table of {ws.R}")
        _, _, out = ws.slack_buffers(_native.slack_group_words(groups.G, ws.R))
        table_ptr = ws.table_ptr if table is ws.table else (ws.send_ptr if table is ws.send else table.data_ptr())
        rc = self.lib.nvrx_slack_group_score(slack_table.data_ptr(), table_ptr, ws.R, ws.K, ws.S, groups.device(self).data_ptr(),
                                             groups.G, groups.max_size, int(min_ranks), int(min_peers), out.data_ptr(),
                                             self._stream_handle)
        if rc < 0:
            _native.check(rc)
        handle = ws._slack_last = SlackGroup(self, out, groups.G, first_rank, n_ranks, int(min_ranks), int(min_peers))
        return handle

    def slack_group_copy_out(self, s: SlackGroup):
        """The one wait of a report's slack scores per peer group: a D2H of the group and pair records and of the rank records
        up to the last rank the report covers, on the backend's stream, behind the kernels."""
        G, rw = s.G, _native.SLACK_RANK_WORDS
        head = _native.SLACK_GROUP_HEAD_WORDS * G
        n = head + rw * (s.first_rank + s.n_ranks)
        host = np.empty(n, dtype=np.uint32)
        _native.check(self.lib.nvrx_d2h_sync(host.ctypes.data, s.d_ptr, n * 4, self._stream_handle))
        return (host[: 8 * G].reshape(G, 8).copy(), host[8 * G: head].reshape(G, _native.SLACK_COLS, 4).copy(),
                host[head + rw * s.first_rank:].reshape(s.n_ranks, rw).copy())

    def row_quantile(self, samples: torch.Tensor, counts: torch.Tensor, q_ppm: int) -> torch.Tensor:
        """Stateless nearest-rank quantile on caller tensors ([rows, stride] f32, [rows] u32/i32) -> [rows] f32, -1.0 where
        a row holds no sample (``nvrx_row_quantile``)."""
        rows, stride = samples.shape
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(self.stream):
            out = torch.empty(max(rows, 1), dtype=torch.float32, device=samples.device)
            _native.check(self.lib.nvrx_row_quantile(samples.data_ptr(), counts.data_ptr(), rows, stride, int(q_ppm),
                                                     out.data_ptr(), self.stream_handle))
        self.stream.synchronize()
        return out[:rows]

    def retire_workspace(self, ws: Workspace) -> None:
        """After a timed-out wait the kernels of ``ws`` may still be queued behind a collective: the workspace
        must neither be reused (stale sequence / ticket state) nor freed under them, so it is parked for good."""
        for key, val in list(self._workspaces.items()):
            if val is ws:
                del self._workspaces[key]
        self._retired.append(ws)

    def synchronize(self) -> None:
        self.stream.synchronize()

    def row_stats(self, samples: torch.Tensor, counts: torch.Tensor, kinds: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Stateless statistics operator on caller tensors ([rows, stride] f32, [rows] u32/i32)."""
        rows, stride = samples.shape
        # the inputs were produced on the caller's current stream; the output is allocated under ours
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(self.stream):
            stats = torch.empty((rows, _native.STATS_STRIDE), dtype=torch.float32, device=samples.device)
            _native.check(
                self.lib.nvrx_row_stats(samples.data_ptr(), counts.data_ptr(), kinds.data_ptr() if kinds is not None else None,
                                        rows, stride, stats.data_ptr(), self.stream_handle)
            )
        self.stream.synchronize()
        return stats


class HipRings:
    """Device ring buffers + pinned staging + hipEvent timing (one ``nvrx_ctx``)."""

    def __init__(self, backend: HipBackend, local_ranks: int, rows_per_rank: int, ring_cap: int):
        self.backend = backend
        self.lib = backend.lib
        self.local_ranks = local_ranks
        self.rows_per_rank = rows_per_rank
        self.ring_cap = ring_cap
        ctx = ctypes.c_void_p()
        _native.check(self.lib.nvrx_ctx_create(backend.device.index, local_ranks, rows_per_rank, ring_cap, ctypes.byref(ctx)))
        self.ctx = ctx
        _native.check(self.lib.nvrx_ctx_set_stream(ctx, backend.stream_handle))
        self._counts_buf = np.zeros(64, dtype=np.int32)
        self._rows_used = 0
        #: every name that ever got a ring row (rows are never recycled; a reset only empties them)
        self.section_row_names = {}
        self.kernel_row_names = {}

    # ---- lifecycle -----------------------------------------------------------------------------
    def close(self) -> None:
        if self.ctx is not None:
            from . import ktrace as _ktrace

            _ktrace.detach_sink_of(self.ctx.value)  # (the kernel tracer's thread must not append to a destroyed context)
            self.lib.nvrx_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # ---- rows ----------------------------------------------------------------------------------
    @property
    def rows_used(self) -> int:
        """Rows handed out so far, as far as the host has been TOLD: the count lives in the library (``nvrx_row_alloc``),
        because the per-kernel tracer's thread takes rows for new kernel keys on its own (``ktrace_sink``); the host's copy
        moves when it allocates a row itself and when the tracer's profiler learns new keys (``note_rows_used``, at
        report time) -- a report covers the rows whose names are known, and reads no C state for it."""
        return self._rows_used

    def note_rows_used(self) -> int:
        """Re-read the library's count (rows the tracer's thread has taken since)."""
        self._rows_used = max(self._rows_used, self.lib.nvrx_ctx_info(self.ctx, 8))
        return self._rows_used

    def alloc_row(self, kind: int = _native.KIND_SECTION) -> int:
        row = self.lib.nvrx_row_alloc(self.ctx, kind)
        if row >= self._rows_used:
            self._rows_used = row + 1
        if row < 0:
            if row == _native.ERR_RANGE:
                raise RuntimeError(
                    f"straggler rings are full: {self.rows_per_rank} timing rows per rank "
                    "(raise max_rows in Detector.initialize)"
                )
            _native.check(row)
        return row

    def row_for(self, kind: int, name: str) -> int:
        """Ring row of a section (kind 0) / GPU-timed region (kind 1), allocated on first use."""
        table = self.kernel_row_names if kind == _native.KIND_KERNEL else self.section_row_names
        row = table.get(name)
        if row is None:
            row = self.alloc_row(kind)
            table[name] = row
        return row

    def ktrace_sink(self):
        """``(ctx, push, row_alloc)`` as plain addresses: what ``nvrx_ktrace_set_sink`` needs to append kernel durations to
        these rings from the tracer's thread (include/nvrx_ktrace.h)."""
        cast = ctypes.cast
        return (self.ctx.value, cast(self.lib.nvrx_sink_push, ctypes.c_void_p).value,
                cast(self.lib.nvrx_sink_row_alloc, ctypes.c_void_p).value)

    def configure(self, row: int, kind: int, gid: int, lr: Optional[int] = None) -> None:
        lrs = range(self.local_ranks) if lr is None else (lr,)
        for q in lrs:
            _native.check(self.lib.nvrx_row_configure(self.ctx, q * self.rows_per_rank + row, kind, gid))

    def push(self, row: int, value: float, lr: int = 0) -> None:
        rc = self.lib.nvrx_ring_push(self.ctx, lr * self.rows_per_rank + row, value)
        if rc < 0:
            _native.check(rc)

    def push_many(self, row: int, values, lr: int = 0) -> None:
        a = np.ascontiguousarray(values, dtype=np.float32)
        _native.check(self.lib.nvrx_ring_push_many(self.ctx, lr * self.rows_per_rank + row, a.ctypes.data, a.size))

    def push_pairs(self, rows: np.ndarray, values: np.ndarray) -> None:
        """Append ``values[i]`` to ring row ``rows[i]`` (global row index; negative = skip) for all i, in order, with
        ONE scatter launch (``nvrx_ring_push_pairs``)."""
        r = np.ascontiguousarray(rows, dtype=np.int32)
        v = np.ascontiguousarray(values, dtype=np.float32)
        if r.size != v.size:
            raise ValueError("rows and values differ in length")
        _native.check(self.lib.nvrx_ring_push_pairs(self.ctx, r.ctypes.data, v.ctypes.data, r.size))

    def push_device(self, row: int, values: torch.Tensor, lr: int = 0) -> None:
        assert values.dtype == torch.float32 and values.is_contiguous() and values.is_cuda
        _native.check(self.lib.nvrx_ring_push_device(self.ctx, lr * self.rows_per_rank + row, values.data_ptr(),
                                                     values.numel(), self.backend.stream_handle))

    def push_device_rows(self, first_row: int, values: torch.Tensor, lr: int = 0) -> None:
        """``values[r]`` appended to row ``first_row + r`` for every r: one call, one strided copy when the rows stand at
        the same ring position."""
        assert values.dtype == torch.float32 and values.is_cuda and values.dim() == 2 and values.stride(1) == 1
        _native.check(self.lib.nvrx_ring_push_device_rows(self.ctx, lr * self.rows_per_rank + first_row, values.shape[0],
                                                          values.data_ptr(), values.shape[1], values.stride(0),
                                                          self.backend.stream_handle))

    def set_count(self, row: int, n: int, lr: int = 0) -> None:
        _native.check(self.lib.nvrx_ring_set_count(self.ctx, lr * self.rows_per_rank + row, n))

    def set_count_all(self, n: int) -> None:
        _native.check(self.lib.nvrx_ring_set_count_all(self.ctx, n))

    def count(self, row: int, lr: int = 0) -> int:
        return _native.check(self.lib.nvrx_ring_count(self.ctx, lr * self.rows_per_rank + row))

    def counts(self) -> np.ndarray:
        """Valid-sample counts of the used rows of logical rank 0 (one C call)."""
        n = self.rows_used
        if self._counts_buf.size < n:
            self._counts_buf = np.zeros(max(n, 64), dtype=np.int32)
        _native.check(self.lib.nvrx_ring_counts(self.ctx, self._counts_buf.ctypes.data, n))
        return self._counts_buf[:n]

    def occupancy_changed(self) -> bool:
        """Whether the SET of used rows that hold samples differs from what the previous call saw (one C call, nothing
        copied): the report's name tables are rebuilt only then."""
        rc = self.lib.nvrx_ring_occupancy_changed(self.ctx, self._rows_used)
        if rc < 0:
            _native.check(rc)
        return rc != 0

    def reset(self) -> None:
        _native.check(self.lib.nvrx_ring_reset(self.ctx))

    def reset_history(self) -> None:
        _native.check(self.lib.nvrx_history_reset(self.ctx, self.backend.stream_handle))

    def flush(self) -> None:
        _native.check(self.lib.nvrx_ring_flush(self.ctx, self.backend.stream_handle))

    def read_row(self, row: int, lr: int = 0) -> np.ndarray:
        stride = _native.check(self.lib.nvrx_ctx_info(self.ctx, 3))
        out = np.empty(stride, dtype=np.float32)
        _native.check(self.lib.nvrx_ring_read(self.ctx, lr * self.rows_per_rank + row, out.ctypes.data, stride,
                                              self.backend.stream_handle))
        return out

    # ---- GPU region timing -----------------------------------------------------------------------
    # (begin / end of a GPU-timed region return False when the region records nothing: its stream is being captured
    #  into a hipGraph -- include/nvrx_straggler.h, NVRX_REGION_SKIPPED)
    def event_begin(self, row: int, stream_handle: int, lr: int = 0) -> bool:
        return _native.check(self.lib.nvrx_event_begin(self.ctx, lr * self.rows_per_rank + row, stream_handle)) == 0

    def event_end(self, row: int, stream_handle: int, lr: int = 0) -> bool:
        return _native.check(self.lib.nvrx_event_end(self.ctx, lr * self.rows_per_rank + row, stream_handle)) == 0

    def harvest(self, wait: bool) -> int:
        return _native.check(self.lib.nvrx_event_harvest(self.ctx, int(wait)))

    # device-side timing: the elapsed time is written into the ring by a kernel on the user's stream
    def stamp_begin(self, row: int, stream_handle: int, lr: int = 0) -> bool:
        rc = self.lib.nvrx_stamp_begin(self.ctx, lr * self.rows_per_rank + row, stream_handle)
        if rc < 0:
            _native.check(rc)
        return rc == 0

    def stamp_end(self, row: int, stream_handle: int, cpu_row: int = -1, cpu_value: float = 0.0, lr: int = 0) -> bool:
        base = lr * self.rows_per_rank
        rc = self.lib.nvrx_stamp_end(self.ctx, base + row, base + cpu_row if cpu_row >= 0 else -1, cpu_value, stream_handle)
        if rc < 0:
            _native.check(rc)
        return rc == 0

    @property
    def regions_skipped(self) -> int:
        """GPU-timed regions that recorded nothing because their stream was being captured into a hipGraph."""
        return int(self.lib.nvrx_ctx_info(self.ctx, 7))

    # ---- report ----------------------------------------------------------------------------------
    def report_local(self, ws: Workspace, names_ok: bool, rows_active: int = 0) -> None:
        """flush -> statistics kernel -> exchange rows, all on the backend's stream (nothing here writes a result block)."""
        if not ws.send_initialised:
            self.backend.send_init(ws)
        rc = self.lib.nvrx_report_local(self.ctx, ws.d_stats, ws.send_ptr, ws.K, ws.S, int(names_ok),
                                        rows_active, self.backend.stream_handle)
        if rc < 0:
            _native.check(rc)

    @staticmethod
    def configure_desc(ws: Workspace, blk: ResultBlock, key: tuple) -> None:
        """Fill a result block's report descriptor for the switches in ``key`` -- ``(rows_active, stats_rows, do_indiv, do_rel,
        thresholds, direct, names_ok, wait, resident)`` -- and remember the key (cold: once per block and shape)."""
        rows_active, stats_rows, do_indiv, do_rel, thresholds, direct, names_ok, wait, resident = key
        d = blk.desc
        d.rows_active, d.stats_rows = rows_active, min(stats_rows, ws.stats_rows)
        d.do_indiv, d.do_rel = int(do_indiv), int(do_rel)
        d.names_ok = int(names_ok)
        for i in range(4):
            d.thresholds[i] = float(thresholds[i])
        if direct is not None:
            d.allgather_fn, d.comm = direct.fn_address, direct.comm_address
        else:
            d.allgather_fn, d.comm = None, None
        d.timeout_s = report_timeout_s()
        d.h_seq_word = blk.h_seq if wait else None
        d.guard_rings = 0 if wait else 1
        # resident score kernel on a stream of its own: the library decides among the eligible shapes (no exchange or
        # peer windows, table fits one workgroup); off when ranks share a device
        d.resident = 1 if (wait and resident) else 0
        blk.desc_key = key

    def _report_prepare(self, ws: Workspace, rows_active: int, stats_rows: int, do_indiv: bool, do_rel: bool,
                        thresholds: Sequence[float], direct, names_ok: bool, wait: bool, order_after: Optional[int],
                        resident: bool, prev_settled: bool) -> ResultBlock:
        """What every form of the one-call report does before its C call: flip to this report's result block, bring its
        descriptor up to date, initialise the exchange rows when they are new.  Returns the block."""
        blk = ws.flip()  # this report's result block; the previous report's block stays readable for one more report
        d = blk.desc
        key = (rows_active, stats_rows, do_indiv, do_rel, thresholds, direct, names_ok, wait, resident)
        if blk.desc_key != key:  # cold: the switches of this shape changed
            self.configure_desc(ws, blk, key)
        # prev_settled: the caller has SEEN this context's previous asynchronous report complete (ReportGenerator polls its
        # completion word in _settle_inflight and says so only when that poll returned): the library may then stop guarding
        # the rings against that report and, when reports are rare, enqueue this one on the stream it has to follow.  A wait
        # that raised, or a caller that never looked, leaves it 0 and the guards stay.
        d.prev_settled = 1 if (prev_settled and not wait) else 0
        if order_after is not None:  # the caller's current stream: the report follows what is enqueued there
            d.order_after_stream, d.order_after_enabled = order_after, 1
        elif d.order_after_enabled:
            d.order_after_enabled = 0
        if not ws.send_initialised:
            self.backend.send_init(ws)
            self.backend.synchronize()  # cold: a resident score kernel touches the exchange rows from its own stream
        d.seq = ws.seq
        return blk

    def report_fused(self, ws: Workspace, rows_active: int, stats_rows: int, do_indiv: bool, do_rel: bool,
                     thresholds: Sequence[float], direct=None, names_ok: bool = True, wait: bool = True,
                     order_after: Optional[int] = None, resident: bool = True, prev_settled: bool = False) -> int:
        """The whole report in one C call (``nvrx_report``): flush -> statistics kernel -> [``ncclAllGather`` of the
        exchange rows through ``direct``] -> score kernel -> wait for the completion word.  On return
        ``ws.scores / flags / meta / stats`` hold this report's values.  ``wait=False`` only enqueues (asynchronous
        report): the caller waits for the returned sequence number with ``backend.wait_seq`` later, and ring writers on
        other streams are ordered after the statistics kernel on the device."""
        blk = self._report_prepare(ws, rows_active, stats_rows, do_indiv, do_rel, thresholds, direct, names_ok, wait,
                                   order_after, resident, prev_settled)
        rc = self.lib.nvrx_report(self.ctx, blk.desc_ref, self.backend._stream_handle)
        ws.seq = blk.desc.seq
        if rc < 0:
            if rc == _native.ERR_TIMEOUT:
                self.backend.retire_workspace(ws)
            _native.check(rc)
        return ws.seq

    def report_issue(self, ws: Workspace, rows_active: int, stats_rows: int, do_indiv: bool, do_rel: bool,
                     thresholds: Sequence[float], direct=None, names_ok: bool = True, order_after: Optional[int] = None,
                     resident: bool = True) -> int:
        """The synchronous ``report_fused`` up to its last launch (``nvrx_report_issue``): everything is enqueued, nothing is
        waited for.  Returns the report's sequence number; ``report_wait(ws)`` must follow, and between the two the caller
        does host work only -- of these rings nothing but ``reset()`` may be called (include/nvrx_straggler.h)."""
        blk = self._report_prepare(ws, rows_active, stats_rows, do_indiv, do_rel, thresholds, direct, names_ok, True,
                                   order_after, resident, False)
        rc = self.lib.nvrx_report_issue(self.ctx, blk.desc_ref, self.backend._stream_handle)
        ws.seq = blk.desc.seq
        if rc < 0:
            _native.check(rc)
        return ws.seq

    def report_wait(self, ws: Workspace) -> None:
        """Wait for the report ``report_issue`` enqueued on ``ws`` (``nvrx_report_wait``).  On return ``ws.scores / flags /
        meta / stats`` hold its values.  When it raises, the block is nobody's -- whatever the caller attached to it in
        between is let go, as if ``report_fused`` had raised -- and a timeout retires the workspace."""
        rc = self.lib.nvrx_report_wait(self.ctx, ws.block.desc_ref)
        if rc < 0:
            ws.block._live = None
            if rc == _native.ERR_TIMEOUT:
                self.backend.retire_workspace(ws)
            _native.check(rc)

    def report_attribute(self, ws: Workspace, top_n: int, first_rank: int = 0, n_ranks: Optional[int] = None) -> Attribution:
        """Kernel attribution of the table of the report ``report_fused`` just issued on ``ws`` (``nvrx_report_attribute``):
        enqueued behind that report's kernels by the library, nothing is waited for."""
        n_ranks = ws.R - first_rank if n_ranks is None else n_ranks
        ws.attr_settle()  # (the records buffer is about to be rewritten; the caller settled before the report already)
        buf, _ = ws.attr_buffers(n_ranks, top_n, False)
        rc = self.lib.nvrx_report_attribute(self.ctx, ws.block.desc_ref, first_rank, n_ranks, top_n, buf.data_ptr())
        if rc < 0:
            _native.check(rc)
        out = ws._attr_last = Attribution(self.backend, buf, first_rank, n_ranks, top_n)
        return out

    def _table_report(self, fam: TableFamily, ws: Workspace, groups: Optional[PeerGroups], first_rank: int,
                      n_ranks: Optional[int], params: tuple) -> TableScores:
        """One table family's scores of the table of the report ``report_fused`` just issued on ``ws``
        (``nvrx_report_<family>``): enqueued behind that report's kernels by the library, nothing is waited for.  (The caller
        settled the workspace before the report already.)"""
        return self.backend._table_step(fam, ws, getattr(self.lib, fam.c_report), (self.ctx, ws.block.desc_ref), (), groups,
                                        first_rank, n_ranks, params)

    # (the families by name: one-line delegations)
    def report_robust(self, ws: Workspace, first_rank: int = 0, n_ranks: Optional[int] = None, min_ranks: int = 4,
                      floor_rel: float = 0.02) -> TableScores:
        return self._table_report(ROBUST, ws, None, first_rank, n_ranks, (min_ranks, floor_rel))

    def report_peer(self, ws: Workspace, groups: PeerGroups, first_rank: int = 0, n_ranks: Optional[int] = None,
                    min_ranks: int = 2) -> TableScores:
        return self._table_report(PEER, ws, groups, first_rank, n_ranks, (min_ranks,))

    def report_pace(self, ws: Workspace, first_rank: int = 0, n_ranks: Optional[int] = None, min_ranks: int = 4) -> TableScores:
        return self._table_report(PACE, ws, None, first_rank, n_ranks, (min_ranks,))

    def report_pace_group(self, ws: Workspace, groups: PeerGroups, first_rank: int = 0, n_ranks: Optional[int] = None,
                          min_ranks: int = 4, min_peers: int = 2) -> TableScores:
        return self._table_report(PACE_GROUP, ws, groups, first_rank, n_ranks, (min_ranks, min_peers))

    def report_node(self, ws: Workspace, nodes: PeerGroups, first_rank: int = 0, n_ranks: Optional[int] = None,
                    min_members: int = 2, min_nodes: int = 3) -> TableScores:
        return self._table_report(NODE, ws, nodes, first_rank, n_ranks, (min_members, min_nodes))

    def report_work(self, ws: Workspace, count_tol: float = 0.25, max_unlike_ppm: int = 100000) -> Work:
        """The work groups of the table of the report ``report_fused`` just issued on ``ws`` (``nvrx_report_work``): enqueued
        behind that report's kernels by the library, nothing is waited for.  (The caller settled the workspace before the
        report already.)"""
        return self.backend._work_step(ws, self.lib.nvrx_report_work, (self.ctx, ws.block.desc_ref), (), count_tol, max_unlike_ppm)

    def report_history(self, ws: Workspace, state: ScoreHistory, first_rank: int = 0, n_ranks: Optional[int] = None,
                       thresholds: Sequence[float] = DEFAULT_THRESHOLDS) -> History:
        """Append the scores of the report ``report_fused`` just issued on ``ws`` to ``state``'s ring
        (``nvrx_report_history``): enqueued behind that report's kernels by the library, nothing is waited for."""
        n_ranks = ws.R - first_rank if n_ranks is None else n_ranks
        be = self.backend
        buf, c_thr = be.history_prepare(ws, state, first_rank, n_ranks, thresholds)
        rc = self.lib.nvrx_report_history(self.ctx, ws.block.desc_ref, first_rank, n_ranks, state.hist.data_ptr(),
                                          state.S_cap, state.depth, state.n_before, c_thr, buf.data_ptr())
        if rc < 0:
            _native.check(rc)
        state.n_before += 1
        out = ws._history_last = History(be, buf, ws.S, first_rank, n_ranks)
        return out

    def report_trend(self, ws: Workspace, state: ScoreHistory) -> Trend:
        """The trends of ``state``'s ring as ``report_history`` just left it (``nvrx_report_trend``): enqueued on the
        context's stream behind that step, nothing is waited for."""
        be = self.backend
        ws.trend_settle()
        n_ranks = state.ranks[1]
        buf = ws.trend_buffers(n_ranks)
        rc = self.lib.nvrx_report_trend(self.ctx, state.hist.data_ptr(), n_ranks, ws.S, state.S_cap, state.depth,
                                        state.n_before, buf.data_ptr())
        if rc < 0:
            _native.check(rc)
        out = ws._trend_last = Trend(be, buf, ws.S, n_ranks)
        return out

    def report_peer_history(self, ws: Workspace, state: PeerHistory, peer: TableScores,
                            thresholds: Sequence[float] = (0.75, 0.75)) -> History:
        """Append the peer scores ``report_peer`` just left in ``ws``'s peer slot (``peer``: that step's handle) to ``state``'s
        ring (``nvrx_report_peer_history``): enqueued on the context's stream directly behind that step, nothing is waited
        for."""
        return self.backend._peer_history_step(ws, state, peer, thresholds, self.lib.nvrx_report_peer_history, (self.ctx,), ())

    def report_peer_trend(self, ws: Workspace, state: PeerHistory) -> Trend:
        """The trends of ``state``'s ring as ``report_peer_history`` just left it (``nvrx_report_peer_trend``): enqueued on the
        context's stream behind that step, nothing is waited for."""
        return self.backend._peer_trend_step(ws, state, self.lib.nvrx_report_peer_trend, (self.ctx,), ())

    _slack_list = None  # (len(kernel_row_names), rows int32, columns int32, {column: keys}): names are only ever added

    def slack_list(self):
        """``(rows, columns, {column: (keys, ...)})`` of the collective kernels' rows, in ascending row order (cached until
        ``kernel_row_names`` grows: rows are never recycled)."""
        cached = self._slack_list
        if cached is None or cached[0] != len(self.kernel_row_names):
            from .reporting import slack_row_list  # (reporting imports this module)

            rows, cols, keys = slack_row_list(self.kernel_row_names)
            cached = self._slack_list = (len(self.kernel_row_names), np.asarray(rows, dtype=np.int32),
                                         np.asarray(cols, dtype=np.int32), keys)
        return cached[1:]

    def slack_local(self, ws: Workspace, rows_active: int = 0, fused: bool = False):
        """The local step of the slack scores on the statistics of the report just issued on ``ws`` (``nvrx_slack_local``;
        ``fused``: that report was ``report_fused``'s, else ``report_local``'s): per logical rank and column the time and the
        calls of the collective rows.  Returns ``(send [local_ranks, 2 * 64], table [R, 2 * 64])`` -- the same rows when
        nothing is exchanged.  Waits for the kernel, as ``tail_local`` does: the next report rewrites the statistics."""
        ws.slack_settle()
        send, table, _ = ws.slack_buffers()
        rows, cols, _ = self.slack_list()
        rc = self.lib.nvrx_slack_local(self.ctx, ws.block.desc_ref if fused else None, ws.d_stats, rows.ctypes.data,
                                       cols.ctypes.data, rows.size, send.data_ptr(), rows_active, self.backend._stream_handle)
        if rc < 0:
            _native.check(rc)
        self.backend.stream.synchronize()
        return send, table

    def _family_local(self, fam: RowFamily, ws: Workspace, params: tuple, rows_active: int, fused: bool):
        """A row family's ring kernel over every ring row as the report just issued on ``ws`` saw it, packed by gid into the
        workspace's rows of that family (``nvrx_<family>_local``; ``fused``: that report was ``report_fused``'s, else
        ``report_local``'s; every family but tail needs ``onset_enable``'s ring-start snapshot).  Returns ``(send
        [local_ranks, P * (K+S)], table [R, P * (K+S)])`` -- the same rows when nothing is exchanged.  Waits for the kernel:
        the rings are emptied by count, and the next window's device-side writers on other streams may overwrite slots as
        soon as the report call returns."""
        assert self.onset_enabled or not fam.needs_starts, f"{fam.name}_local() before onset_enable(): no ring-start snapshot"
        ws.family_settle(fam)
        send, table, _, _ = ws.family_buffers(fam)
        rc = getattr(self.lib, fam.c_local)(self.ctx, ws.block.desc_ref if fused else None, int(params[0]),
                                            *map(float, params[1:]), send.data_ptr(), ws.K, ws.S, rows_active,
                                            self.backend._stream_handle)
        if rc < 0:
            _native.check(rc)
        self.backend.stream.synchronize()
        return send, table

    def tail_local(self, ws: Workspace, q_ppm: int, rows_active: int = 0, fused: bool = False):
        return self._family_local(TAIL, ws, (q_ppm,), rows_active, fused)

    onset_enabled = False

    def onset_enable(self, on: bool = True) -> None:
        """From now on every report also notes where each ring's oldest sample lives (``nvrx_onset_enable``): what the
        families that walk the report's window in time order need."""
        _native.check(self.lib.nvrx_onset_enable(self.ctx, int(on)))
        self.onset_enabled = bool(on)

    def onset_local(self, ws: Workspace, min_seg_ppm: int, min_strength: float, rows_active: int = 0, fused: bool = False):
        return self._family_local(ONSET, ws, (min_seg_ppm, min_strength), rows_active, fused)

    def period_local(self, ws: Workspace, max_period: int, min_strength: float, rows_active: int = 0, fused: bool = False):
        return self._family_local(PERIOD, ws, (max_period, min_strength), rows_active, fused)

    def episode_local(self, ws: Workspace, min_len_ppm: int, min_strength: float, rows_active: int = 0, fused: bool = False):
        return self._family_local(EPISODE, ws, (min_len_ppm, min_strength), rows_active, fused)

    def peek_stats(self) -> np.ndarray:
        """Statistics of every used row right now ([rows_used, 8] on the host); exchanges nothing and
        leaves the history minima alone."""
        total = self.local_ranks * self.rows_per_rank
        # allocated, written and read under the backend's stream: the caching allocator then never hands out a block
        # that kernels on the user's current stream may still be using
        with torch.cuda.stream(self.backend.stream):
            stats = torch.empty((total, _native.STATS_STRIDE), dtype=torch.float32, device=self.backend.device)
            _native.check(self.lib.nvrx_report_local(self.ctx, stats.data_ptr(), None, 0, 0, 1, self.rows_used,
                                                     self.backend.stream_handle))
            host = stats.cpu()
        self.backend.stream.synchronize()
        return host.numpy()

    def timing_enable(self, on: bool) -> None:
        _native.check(self.lib.nvrx_timing_enable(self.ctx, int(on)))

    def timing_read(self, reset: bool = True):
        total = ctypes.c_double()
        launches = ctypes.c_int()
        _native.check(self.lib.nvrx_timing_read(self.ctx, ctypes.byref(total), ctypes.byref(launches), int(reset)))
        return total.value, launches.value
