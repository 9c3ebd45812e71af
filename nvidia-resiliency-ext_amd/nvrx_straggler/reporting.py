"""Performance report of the straggler detector: cross-rank exchange, on-device scoring, thresholds.

Public surface kept from the reference (reporting.py): ``StragglerId`` (:31-38), ``Report`` with its
10 fields (:41-82) and ``identify_stragglers`` (:84-151), and ``ReportGenerator(scores_to_compute,
gather_on_rank0=True, pg=None, node_name='<notset>').generate_report(section_summaries,
kernel_summaries)`` (:154-554).

What is different underneath (MI355X-first):

* a report is ONE fixed-length all-gather of every rank's exchange row -- medians, running minima,
  kernel weights and a "names complete" flag -- instead of the reference's all_reduce(MIN) flag +
  all_reduce(MIN) medians + gather of scores (three collectives with host<->device copies around
  each);
* every score for every rank, and the below-threshold flags, come from one HIP kernel over the
  gathered table (``nvrx_score``); the host never loops over kernels or sections;
* one small D2H copy brings back scores + flags + local statistics; ``Report`` exposes them through
  lazy mapping views so nothing is converted to Python objects until it is read.

Scores therefore pass through f32 (as the reference's gathered scores do, reporting.py:352).
"""
from __future__ import annotations

import collections
import dataclasses
import itertools
import logging
import math
import os
import threading
import time
from typing import Any, Dict, List, Mapping, Optional, Sequence

import numpy as np

from . import backend as _backend_mod
from . import dist_utils, row_families
from .name_mapper import NameMapper, name_digest
from .statistics import NUM_COLUMN, STAT_KEYS, Statistic

_SummaryType = Mapping[Statistic, float]
_LOG = logging.getLogger(__name__)



def _load_pyread():
    """csrc/nvrx_pyread.c: the same dicts without numpy's intermediate lists (host-side formatting only; same results).
    ``NVRX_DEBUG_LIB_DIR`` (the sanitizer builds, tools/run_sanitized.sh) may hold its own build of it, which then wins."""
    alt = os.environ.get("NVRX_DEBUG_LIB_DIR", "")
    if alt:
        import glob
        import importlib.util

        for path in sorted(glob.glob(os.path.join(alt, "_nvrx_pyread*.so"))):
            spec = importlib.util.spec_from_file_location(f"{__package__}._nvrx_pyread", path)
            if spec is not None and spec.loader is not None:
                try:
                    mod = importlib.util.module_from_spec(spec)
                    spec.loader.exec_module(mod)
                except (ImportError, OSError) as e:  # a stale / ABI-mismatched file there: the packaged module, or Python
                    _LOG.warning("ignoring %s: %s", path, e)
                    continue
                return mod
    try:
        from . import _nvrx_pyread
    except ImportError:  # not built: the Python builders below
        return None
    return _nvrx_pyread


_pyread = _load_pyread()
# (said once, at INFO: which of the three formatting paths -- all with the same results -- this interpreter gets)
if _pyread is None:
    _LOG.info("nvrx straggler: csrc/nvrx_pyread.c is not built for this interpreter; a report's dicts are built by the Python "
              "builders (same results, slower reads)")
else:
    try:
        if not _pyread.inplace():
            import sys as _sys

            _LOG.info("nvrx straggler: the in-place fill of a report's cloned dicts follows CPython 3.10's dict layout; Python %d.%d "
                      "uses the public dict API instead (same results, ~10 us more per fully read 8 x 64 report)", *_sys.version_info[:2])
    except Exception:  # noqa: BLE001  (an older build of the helper without the query)
        pass


def _copy_sets(d: Dict[str, set]) -> Dict[str, set]:
    """``{name: set}`` copied one level deep (callers of ``identify_stragglers`` may do what they like with their sets)."""
    if _pyread is not None:
        return _pyread.copy_sets(d)
    return {n: v.copy() for n, v in d.items()}

# Kernels of the collective library are kept out of the GPU score: their duration is peer-wait time.  The reference
# drops every key containing "ncclDev" (reporting.py:330-336), which on CUDA matches NCCL's ncclDevKernel_* family.
# RCCL's device kernels are named differently -- rcclGenericKernel<N, bool>(ncclDevKernelArgsStorage<4096>) and
# mscclKernel_<op>_<type>_<proto>_<bool>(ncclDevComm*, mscclAlgo*, mscclWork*) -- and the keys here carry MANGLED
# names, where the argument types appear, so the reference's substring still hits every one of them
# (tests/test_host_logic.py::test_rccl_kernel_names_of_the_installed_library_are_filtered reads the names out of the
# installed librccl.so).  The two RCCL family names are matched as well, so the filter does not depend on an argument
# type staying in the signature.
_NCCL_MARKER = "ncclDev"
_COLLECTIVE_MARKERS = (_NCCL_MARKER, "rcclGenericKernel", "mscclKernel")


def is_collective_kernel(name: str) -> bool:
    return _NCCL_MARKER in name or "rcclGenericKernel" in name or "mscclKernel" in name


SLACK_COLS = 64  # NVRX_SLACK_COLS (include/nvrx_straggler.h)


def slack_column(key: str) -> int:
    """The column of the slack scores that a collective kernel's key falls into: the same on every rank, from the key alone
    -- nothing is agreed between ranks, so no name sync can hang on it.  Keys that collide share a column."""
    return name_digest(key) % SLACK_COLS


def slack_row_list(kernel_row_names: Mapping[str, int]):
    """``(rows, columns, {column: (keys, ...)})`` of the collective kernels among ``kernel_row_names`` (key -> ring row), in
    ascending row order: what the local step of the slack scores walks."""
    pairs = sorted((row, slack_column(key), key) for key, row in kernel_row_names.items() if is_collective_kernel(key))
    keys: Dict[int, tuple] = {}
    for _, col, key in pairs:
        keys[col] = keys.get(col, ()) + (key,)
    return [p[0] for p in pairs], [p[1] for p in pairs], keys


@dataclasses.dataclass(frozen=True)
class StragglerId:
    """Identity of a flagged rank: global rank and the node it runs on."""

    rank: int
    node: str


# --------------------------------------------------------------------------------------------------
# Report: a frozen record of plain dicts, some of them built on first read
# --------------------------------------------------------------------------------------------------
def _row_selector(rows: Mapping[str, int]):
    """How to cut ``rows``' statistics out of the block: a slice when the rows are consecutive (ring rows are handed
    out in order of first use, so they nearly always are), else an index array."""
    idx = list(rows.values())
    if idx and idx == list(range(idx[0], idx[0] + len(idx))):
        return slice(idx[0], idx[0] + len(idx))
    return np.asarray(idx, dtype=np.intp)


def _summaries_from_rows(rows: Mapping[str, int], stats: np.ndarray, selector=None, name_template=None,
                         recycle=None, tuples=None) -> Dict[str, Dict[Statistic, Any]]:
    """``name -> {Statistic: value}`` from device statistics rows (``_get_section_summaries``' result shape,
    straggler.py:185-195), NUM as an integer as in the reference (straggler.py:194).  Built by ``_nvrx_pyread`` when it
    is there; else one C-level conversion of the whole block and one ``dict(zip(keys, row))`` per name (``Statistic``
    hashes by identity)."""
    if not rows:
        return {}
    if _pyread is not None and stats.dtype == np.float32 and stats.flags.c_contiguous and stats.shape[1] == 8:
        names, idx = tuples if tuples is not None else (tuple(rows), tuple(rows.values()))
        return _pyread.summaries(names, STAT_KEYS, stats, idx, name_template, recycle)
    block = stats[_row_selector(rows) if selector is None else selector]
    vals = block[:, : NUM_COLUMN + 1].tolist()
    out = dict(zip(rows, map(dict, map(zip, itertools.repeat(STAT_KEYS), vals))))
    num = Statistic.NUM
    counts = block[:, NUM_COLUMN]
    if not np.isfinite(counts).all():  # cannot come out of the statistics kernel; the C builder raises here too
        raise ValueError("cannot convert a non-finite NUM statistic to an integer")
    for d, n in zip(out.values(), counts.astype(np.int64).tolist()):
        d[num] = n
    return out


class _PendingBlock:
    """Result block of a report the host has not waited for (asynchronous reports): the kernels are enqueued, the
    pinned block fills in when they run.  ``complete()`` polls the completion word and leaves the data where it is;
    ``wait()`` also takes the private copy -- when the report is first read, or (``detach``, called by the block) before
    the block is written again, two reports later, if somebody still holds the report.  An asynchronous report that is
    never read therefore costs its successor one poll of a word that has long been written, not a copy of the block: at
    production cadence that copy ran cold and was half of what enqueueing the next report cost (47 of 95 us,
    profiles/r04f_cadence_breakdown.txt)."""

    __slots__ = ("backend", "ws", "blk", "seq", "blob", "lock", "__weakref__")

    def __init__(self, backend, ws, seq: int):
        self.backend, self.ws, self.seq = backend, ws, seq
        self.blk = getattr(ws, "block", None)  # the one of the workspace's result blocks this report was enqueued into
        self.blob: Optional[np.ndarray] = None
        self.lock = threading.Lock()
        if self.blk is not None:
            self.blk.attach(self)  # the block collects this report (if still held) before anything writes it again

    def complete(self) -> int:
        """Wait until the report has published its results; returns its ``names complete`` word (meta[0])."""
        with self.lock:
            blk = self.blk
            if self.blob is None and blk is not None:
                words = getattr(blk, "meta_words", None)
                if words is None:  # (the CPU checker backend's block)
                    self.backend.wait_seq(self.ws, self.seq, block=blk)
                    return int(blk.meta[0])
                if words[4] != self.seq:  # (usually published long ago: one look at the word, no call)
                    self.backend.wait_seq(self.ws, self.seq, block=blk)
                return words[0]
        return int(self.wait()[0:4].view(np.uint32)[0])

    def wait(self) -> np.ndarray:
        with self.lock:
            if self.blob is None:
                if self.blk is not None:
                    self.backend.wait_seq(self.ws, self.seq, block=self.blk)
                    self.blob = self.blk.host_block()
                else:  # (the CPU checker backend of the tests: one block, computed at enqueue time)
                    self.backend.wait_seq(self.ws, self.seq)
                    self.blob = self.ws.host_block()
                self.backend = self.ws = self.blk = None  # nothing of the live workspace is referenced any more
        return self.blob

    def detach(self) -> None:
        self.wait()


_LIVE_LOCK = threading.Lock()  # a report may be read on another thread while the generator collects it


class _LiveBlock:
    """The result block of a synchronous one-call report, still in place.  Nothing is copied when the report returns:
    ``head()`` / ``stats()`` take private copies when the report is first read, and the block calls ``detach()`` before
    anything writes it again -- two reports later (a workspace alternates between two blocks), and it copies only if
    somebody still holds the report by then.  The statistics rows have a completion word of their own (a resident
    score kernel forwards them after the scores)."""

    __slots__ = ("backend", "ws", "blk", "seq", "rows", "_head", "_head_bytes", "_stats", "__weakref__")

    def __init__(self, backend, ws, seq: int, rows: int):
        self.backend, self.ws, self.seq, self.rows = backend, ws, seq, rows
        self.blk = getattr(ws, "block", ws)  # (the CPU checker backend's workspace is its own single block)
        self._head: Optional[np.ndarray] = None
        self._head_bytes: Optional[bytes] = None
        self._stats: Optional[np.ndarray] = None

    def head_bytes(self) -> bytes:
        """meta | scores | flags as ONE ``bytes`` copy of the block (a single memcpy; the flag path of
        ``identify_stragglers`` needs nothing else of the block and nothing of numpy)."""
        if self._head_bytes is None:
            with _LIVE_LOCK:
                if self._head_bytes is None:
                    grab = getattr(self.blk, "host_head_bytes", None)
                    self._head_bytes = grab() if grab is not None else self.blk.host_head().tobytes()
                    self._release()
        return self._head_bytes

    def head(self) -> np.ndarray:
        if self._head is None:
            self._head = np.frombuffer(self.head_bytes(), dtype=np.uint8)  # read-only view of the private copy
        return self._head

    def stats(self) -> np.ndarray:
        if self._stats is None:
            with _LIVE_LOCK:
                if self._stats is None:
                    if self.blk is self.ws:
                        self.backend.wait_seq(self.ws, self.seq, stats=True)
                    else:
                        self.backend.wait_seq(self.ws, self.seq, stats=True, block=self.blk)
                    self._stats = self.blk.host_stats(self.rows)
                    self._release()
        return self._stats

    def in_place(self, fn, stats: bool):
        """``fn(the block's pinned bytes)`` while the block is still this report's -- nothing is copied, not even for the
        mapping builders: under the lock the generator cannot collect this report (``detach`` takes it too), and until it
        has, nothing is enqueued that writes the block again.  ``stats``: the statistics rows are what is read (they have a
        completion word of their own).  None when a private copy exists already or the block exports no flat buffer."""
        with _LIVE_LOCK:
            blk = self.blk
            if blk is None or (self._stats if stats else self._head_bytes) is not None:
                return None
            live = getattr(blk, "_host", None)
            if live is None:
                return None
            if stats:
                if blk is self.ws:
                    self.backend.wait_seq(self.ws, self.seq, stats=True)
                else:
                    self.backend.wait_seq(self.ws, self.seq, stats=True, block=blk)
            try:
                return fn(live)
            except (BufferError, TypeError):
                return None

    def detach(self) -> None:
        self.head_bytes()
        self.stats()

    def _release(self) -> None:
        if self._head_bytes is not None and self._stats is not None:
            self.backend = self.ws = self.blk = None  # nothing of the live workspace is referenced any more


class _View:
    """What all reports of one plan share (immutable once built): table shape, rank / name tables, which score families
    exist, where this report's rows sit in the result block, the thresholds the score kernel flagged with."""

    __slots__ = ("S", "ranks", "names", "cols", "has_rel", "has_indiv", "section_rows", "kernel_rows", "layout", "thresholds",
                 "_rank_list", "_col_index", "_selectors", "_ids", "_memo", "_tuples", "_flag_args")

    def memo(self) -> dict:
        try:
            return self._memo
        except AttributeError:
            self._memo = {}
            return self._memo

    def flag_memo(self) -> list:
        """[flag bytes, (ids, gpu_rel, gpu_indiv, sec_rel, sec_indiv, ...), newest, older] of the last flag table
        ``_nvrx_pyread.flagged`` decoded for this plan, and the last two results it handed out: an unchanged table's sets
        are handed out again once their caller has dropped them, as copies otherwise."""
        m = self.memo()
        try:
            return m["c"]
        except KeyError:
            m["c"] = [None, None, None, None]
            return m["c"]

    def rank_list(self) -> list:
        try:
            return self._rank_list
        except AttributeError:
            self._rank_list = list(self.ranks)
            return self._rank_list

    def rank_tuple(self) -> tuple:
        try:
            return self._tuples[0]
        except AttributeError:
            idx = self.col_index()
            self._tuples = (tuple(self.ranks), tuple(self.names), None if idx is None else tuple(int(i) for i in idx))
            return self._tuples[0]

    def names_tuple(self) -> tuple:
        self.rank_tuple()
        return self._tuples[1]

    def col_tuple(self):
        self.rank_tuple()
        return self._tuples[2]

    def name_template(self, which: str = "names"):
        """``{name: None}`` over the view's section names (``names``) or over the names of its section / kernel rows:
        ``_nvrx_pyread`` clones it for the outer dict of a mapping instead of inserting the names one by one (the template
        itself is never handed out and never modified)."""
        try:
            return self._memo[("tmpl", which)]
        except (AttributeError, KeyError):
            src = self.names if which == "names" else getattr(self, which)
            t = self.memo()[("tmpl", which)] = dict.fromkeys(src)
            return t

    def row_tuples(self, which: str):
        """``(names, rows)`` of ``section_rows`` / ``kernel_rows`` as the two tuples ``_nvrx_pyread.summaries`` takes."""
        try:
            return self._memo[("rows", which)]
        except (AttributeError, KeyError):
            rows = getattr(self, which)
            t = self.memo()[("rows", which)] = (tuple(rows), tuple(rows.values()))
            return t

    def recycle_list(self, which: str, slots: int = 1):
        """The last mapping(s) ``_nvrx_pyread`` built for this plan: when nothing else refers to one any more (the report it
        was built for is gone and nobody kept the dict) the next report's mapping is that very object with its values
        swapped -- see csrc/nvrx_pyread.c, "recycling".  A list per kind of mapping, owned by the plan's memo."""
        try:
            return self._memo[("recycle", which)]
        except (AttributeError, KeyError):
            lst = self.memo()[("recycle", which)] = [None] * slots
            return lst

    def col_index(self):
        """Score-table column of every name of ``names``, in that order (None: the identity)."""
        try:
            return self._col_index
        except AttributeError:
            idx = [self.cols[n] for n in self.names]
            self._col_index = None if idx == list(range(self.S)) else np.asarray(idx, dtype=np.intp)
            return self._col_index

    def selector(self, which: str):
        try:
            sel = self._selectors
        except AttributeError:
            sel = self._selectors = {}
        if which not in sel:
            sel[which] = _row_selector(getattr(self, which))
        return sel[which]

    def straggler_ids(self, rank_to_node) -> list:
        """``StragglerId`` of every row of this view's score table (built once per ``rank_to_node`` object: the
        generator hands the same dict to every report of a plan)."""
        try:
            owner, ids = self._ids
            if owner is rank_to_node:
                return ids
        except AttributeError:
            pass
        ids = [StragglerId(rank=r, node=rank_to_node[r]) for r in self.ranks]
        self._ids = (rank_to_node, ids)
        return ids


class _ScoreSource:
    """What a steady-state report keeps of the result block: the (shared, immutable) view of its plan and the block
    itself -- live, in flight or a private copy.  The six mapping fields of ``Report`` are built from it as PLAIN
    dicts the first time each one is read; a report whose scores are only thresholded (``identify_stragglers`` with
    the kernel's thresholds) never builds any.  The arrays are cut out of the block on first use."""

    __slots__ = ("view", "pending", "scores", "stats", "flags")

    def __init__(self, view: _View, pending=None):
        self.view = view
        self.pending = pending  # ndarray (private copy), _LiveBlock (synchronous report) or _PendingBlock (asynchronous)
        self.scores = self.stats = self.flags = None

    def cut(self, blob: np.ndarray) -> None:
        """Views of this report's scores / flags / statistics inside a private copy of the result block."""
        off_s, off_f, off_t, R, W, lo, hi, stats_rows = self.view.layout
        self.scores = blob[off_s : off_s + R * W * 4].view(np.float32).reshape(R, W)[lo:hi]
        self.flags = blob[off_f : off_f + R * W].reshape(R, W)[lo:hi]
        if blob.size >= off_t + stats_rows * 32:  # a copy of the whole block; else the statistics come later
            self.stats = blob[off_t : off_t + stats_rows * 32].view(np.float32).reshape(stats_rows, 8)

    def statistics(self) -> np.ndarray:
        st = self.stats
        if st is None:
            pend = self.pending
            if self.scores is None and type(pend) is _LiveBlock:
                st = pend  # (a live block hands its statistics rows out on their own: no cut of the head needed for them)
            else:
                self.ensure()
                st = self.stats
        if type(st) is _LiveBlock:
            st = self.stats = st.stats()
        return st

    def raw_scores(self):
        """``(buffer, byte offset, rows, width)`` of this report's score rows for ``_nvrx_pyread`` -- for a live block its
        ``bytes`` copy of the head, addressed by offset: no numpy view is cut for a report whose mappings are built in C."""
        if self.scores is None and type(self.pending) is _LiveBlock:
            off_s, _, _, _, W, lo, hi, _ = self.view.layout
            return self.pending.head_bytes(), off_s + lo * W * 4, hi - lo, W
        sc = self.ensure().scores
        if sc.dtype == np.float32 and sc.flags.c_contiguous:
            return sc, 0, sc.shape[0], sc.shape[1]
        return None

    def ensure(self) -> "_ScoreSource":
        if self.scores is None:
            pend = self.pending
            if pend is not None:
                t = type(pend)
                if t is _LiveBlock:
                    self.stats = pend  # resolved by statistics()
                    self.cut(pend.head())
                else:
                    self.cut(pend if t is np.ndarray else pend.wait())
                self.pending = None
        return self

    def flag_bytes(self) -> bytes:
        """This report's flag rows ([ranks, 2+2S] u8, row-major) as ``bytes``."""
        if self.scores is None and type(self.pending) is _LiveBlock:
            _, off_f, _, _, W, lo, hi, _ = self.view.layout
            return self.pending.head_bytes()[off_f + lo * W : off_f + hi * W]
        return self.ensure().flags.tobytes()

    def flagged(self, rank_to_node, thresholds):
        """``identify_stragglers`` at the thresholds the score kernel flagged with, decoded by ``_nvrx_pyread.flagged``
        straight from the flag bytes (None: other thresholds, or the helper was not built -- the caller's general path).
        One Python frame and one C call: a report read once a minute runs all of this cold."""
        v = self.view
        if _pyread is None or thresholds != v.thresholds:
            return None
        try:
            owner, off, args = v._flag_args
        except AttributeError:
            owner = None
        if owner is not rank_to_node:  # once per plan: the generator hands the same rank_to_node to all its reports
            _, off_f, _, _, W, lo, hi, _ = v.layout
            off = off_f + lo * W
            args = (hi - lo, W, v.S, v.has_rel, v.has_indiv, v.straggler_ids(rank_to_node), v.names_tuple(), v.col_tuple(),
                    v.flag_memo())
            v._flag_args = (rank_to_node, off, args)
        pend = self.pending
        out = None
        if self.scores is None and type(pend) is _PendingBlock:
            # an asynchronous report read late: its flags are decoded in place as well -- the report's own lock keeps the
            # block from collecting it (``detach``), and until it has, nothing is enqueued that writes the block again
            with pend.lock:
                blk = pend.blk
                live = getattr(blk, "_host", None) if (pend.blob is None and blk is not None) else None
                if live is not None:
                    pend.backend.wait_seq(pend.ws, pend.seq, block=blk)
                    try:
                        out = _pyread.flagged(live, off, *args)
                    except (BufferError, TypeError):
                        out = None
        if out is not None:
            pass
        elif self.scores is None and type(pend) is _LiveBlock:
            with _LIVE_LOCK:
                # the result block itself, nothing copied: under the lock the generator cannot collect this report
                # (``detach`` takes it too), and until it has, nothing is enqueued that writes the block again
                blk = pend.blk
                live = getattr(blk, "_host", None) if pend._head_bytes is None else None
                if live is not None:
                    try:
                        out = _pyread.flagged(live, off, *args)
                    except (BufferError, TypeError):  # a block that does not export a flat byte buffer: its private copy
                        out = None
            if out is None:
                out = _pyread.flagged(pend.head_bytes(), off, *args)
        else:
            buf = self.ensure().flags
            out = _pyread.flagged(buf if buf.flags.c_contiguous else np.ascontiguousarray(buf), 0, *args)
        return {"straggler_gpus_relative": out[0], "straggler_gpus_individual": out[1],
                "straggler_sections_relative": out[2], "straggler_sections_individual": out[3]}

    def device_flags(self) -> "_DeviceFlags":
        v = self.view
        return _DeviceFlags(v.thresholds, self, v.ranks, v.names, v.cols, v.S, v.has_rel, v.has_indiv)

    def build(self, field: str, stash: Optional[dict] = None):
        """One of the six mappings as a plain dict.  ``stash``: the report's ``__dict__`` -- a call that can build a
        sibling in the same pass (both section-score families share names, ranks and hashes) leaves it there."""
        v = self.view
        if field == "local_section_summaries" or field == "local_kernel_summaries":  # (nothing of the score rows is needed)
            which = "section_rows" if field == "local_section_summaries" else "kernel_rows"
            rows = getattr(v, which)
            if not rows:
                return {}
            live = self.stats if self.stats is not None else self.pending
            if _pyread is not None and type(live) is _LiveBlock and (self.scores is None or self.stats is live):
                # the statistics rows straight out of the result block: no numpy copy of them for a report that only builds dicts
                names, idx = v.row_tuples(which)
                off_t = v.layout[2]
                out = live.in_place(lambda buf: _pyread.summaries(names, STAT_KEYS, buf, idx, v.name_template(which),
                                                                  v.recycle_list(which), off_t), True)
                if out is not None:
                    return out
            return _summaries_from_rows(rows, self.statistics(), v.selector(which), v.name_template(which), v.recycle_list(which),
                                        v.row_tuples(which))
        if _pyread is not None:
            # (the score rows are NOT read in place from a live block: the builders walk them column by column, and strided
            #  reads of the pinned, device-mapped block cost the CPU twice what one sequential copy of the head + reads of
            #  the copy cost -- 12.0 against 6.7 us for both section families, tools/report_read_fields.py)
            raw = self.raw_scores()
            if raw is not None:
                return self._score_field(field, stash, *raw)
        sc = self.ensure().scores
        if field == "gpu_relative_perf_scores" or field == "gpu_individual_perf_scores":
            col = 1 if field == "gpu_relative_perf_scores" else 0
            if not (v.has_rel if col else v.has_indiv):
                return {}
            return dict(zip(v.ranks, sc[:, col].tolist()))
        if field == "section_relative_perf_scores" or field == "section_individual_perf_scores":
            rel = field == "section_relative_perf_scores"
            if not ((v.has_rel if rel else v.has_indiv) and v.names):
                return {}
            return self._sections(2 + v.S if rel else 2)
        raise AttributeError(field)

    def _score_field(self, field: str, stash: Optional[dict], buf, off: int, nrows: int, W: int):
        """A score mapping built by ``_nvrx_pyread`` from the [nrows, W] f32 rows at ``buf + off``; never None."""
        v = self.view
        S = v.S
        if field == "gpu_relative_perf_scores" or field == "gpu_individual_perf_scores":
            col = 1 if field == "gpu_relative_perf_scores" else 0
            if not (v.has_rel if col else v.has_indiv):
                return {}
            rt = v.rank_tuple()
            other = "gpu_individual_perf_scores" if col else "gpu_relative_perf_scores"
            if stash is not None and other not in stash and (v.has_indiv if col else v.has_rel):
                stash[other] = _pyread.ranks(rt, buf, off, nrows, W, 1 - col)  # the sibling costs one more C call now, no frame later
            return _pyread.ranks(rt, buf, off, nrows, W, col)
        if field == "section_relative_perf_scores" or field == "section_individual_perf_scores":
            rel = field == "section_relative_perf_scores"
            if not ((v.has_rel if rel else v.has_indiv) and v.names):
                return {}
            other = "section_individual_perf_scores" if rel else "section_relative_perf_scores"
            if stash is not None and other not in stash and (v.has_indiv if rel else v.has_rel):
                mine, sibling = _pyread.sections(v.names_tuple(), v.rank_tuple(), buf, off, nrows, W,
                                                 2 + S if rel else 2, v.col_tuple(), 2 if rel else 2 + S, v.name_template(),
                                                 v.recycle_list("sections", 2))
                stash[other] = sibling
                return mine
            return _pyread.sections(v.names_tuple(), v.rank_tuple(), buf, off, nrows, W, 2 + S if rel else 2, v.col_tuple(), -1,
                                    v.name_template(), v.recycle_list("sections", 2))
        raise AttributeError(field)

    def _sections(self, first_col: int) -> Dict[str, Dict[int, float]]:
        """``section -> {rank: score}`` (reporting.py:196-217 builds the same shape score by score): ``_nvrx_pyread``
        walks the [ranks, 2+2S] block directly; without it, one C-level conversion of the [S, ranks] block and one
        ``dict(zip(...))`` per section."""
        v = self.view
        sc = self.scores
        idx = v.col_index()
        if _pyread is not None and sc.dtype == np.float32 and sc.flags.c_contiguous:
            return _pyread.sections(v.names_tuple(), v.rank_tuple(), sc, 0, sc.shape[0], sc.shape[1], first_col, v.col_tuple(), -1,
                                    v.name_template())
        block = sc[:, first_col : first_col + v.S].T
        if idx is not None:
            block = block[idx]
        return dict(zip(v.names, map(dict, map(zip, itertools.repeat(v.rank_list()), block.tolist()))))


class _AttrSource:
    """What a report keeps of its kernel attribution: the backend's handle (``records()`` waits for the kernel and copies the
    records out on first use), the ranks its rows stand for, which families were computed, and the kernel names by id as
    the report's mapper had them at report time (ids are never reassigned)."""

    __slots__ = ("handle", "ranks", "names", "has_rel", "has_indiv", "_built")

    def __init__(self, handle, ranks, names, has_rel: bool, has_indiv: bool):
        self.handle, self.ranks, self.names = handle, tuple(ranks), names
        self.has_rel, self.has_indiv = has_rel, has_indiv
        self._built: Optional[dict] = None

    def build(self) -> dict:
        if self._built is None:
            rec = np.ascontiguousarray(self.handle.records(), dtype=np.uint32)
            f32 = rec.view(np.float32)
            ids = rec.view(np.int32)[:, :, 1:, 0]
            out: Dict[str, Dict[int, Any]] = {}
            for fam, key, on in ((1, "relative", self.has_rel), (0, "individual", self.has_indiv)):
                if not on:
                    continue
                per_rank = out[key] = {}
                for i, rank in enumerate(self.ranks):
                    head = f32[i, fam, 0]
                    kernels = [{"kernel": self.names[k], "share": float(e[1]), "score": float(e[2]), "lost_us": float(e[3])}
                               for k, e in zip(ids[i, fam].tolist(), f32[i, fam, 1:]) if k >= 0]
                    per_rank[rank] = {"deficit": float(head[0]), "explained": float(head[1]),
                                      "num_kernels": int(rec[i, fam, 0, 2]), "kernels": kernels}
            self._built = out
            self.handle = None
        return self._built


def _copy_explanation(d: dict) -> dict:
    return {fam: {r: dict(v, kernels=[dict(k) for k in v["kernels"]]) for r, v in ranks.items()} for fam, ranks in d.items()}


class _RowFamilySource:
    """What a report keeps of one row family's scores (row_families.py: tail, onset, period, episode): the backend's handle
    (``records()`` waits for the kernels and copies the planes and scores out on first use), the ranks its rows stand for,
    the sections it shows with their ids, the kernel names by id as the report's mapper had them at report time, and the
    family's parameters."""

    __slots__ = ("family", "handle", "ranks", "sections", "kernels", "params", "_built")

    def __init__(self, family, handle, ranks, sections, kernels, params: tuple):
        self.family, self.handle, self.ranks, self.kernels, self.params = family, handle, tuple(ranks), kernels, params
        self.sections = {n: g for n, g in sections.items() if g is not None}  # (a name whose id is still to be agreed has no column)
        self._built: Optional[dict] = None

    def build(self) -> dict:
        if self._built is None:
            fam, params, ranks = self.family, self.params, self.ranks
            planes, scores = self.handle.records()
            K, P, record = len(self.kernels), fam.planes, fam.record
            o, sc = planes.reshape(len(ranks), P, -1).tolist(), scores.tolist()

            def present(col):
                out = {}
                for i, r in enumerate(ranks):
                    rec = record([o[i][p][col] for p in range(P)], params)
                    if rec is not None:
                        out[r] = rec
                return out

            kernel_records = {name: present(k) for k, name in enumerate(self.kernels)}
            section_records = {name: present(K + g) for name, g in self.sections.items()}
            built = fam.footer(params) if fam.footer_first else {}
            built.update({
                "gpu_relative": {r: sc[i][0] for i, r in enumerate(ranks)},
                "section_relative": {name: {r: sc[i][1 + g] for i, r in enumerate(ranks)} for name, g in self.sections.items()},
                "section_" + fam.stem: {n: v for n, v in section_records.items() if v},
                "kernel_" + fam.stem: {n: v for n, v in kernel_records.items() if v},
            })
            if not fam.footer_first:
                built.update(fam.footer(params))
            for alias, key in fam.aliases:
                built[alias] = built[key]
            self._built = built
            self.handle = None
        return self._built


class _RowGroupFamilySource(_RowFamilySource):
    """What a report keeps of one row family's scores per peer group (``ReportGenerator(row_peer_groups=True)``):
    ``_RowFamilySource``'s, the resolved groups and ``min_peers``.  The handle's ``records()`` delivers the column records
    ``[G][K+S]`` as well."""

    __slots__ = ("groups", "min_peers")

    def __init__(self, family, handle, ranks, sections, kernels, params: tuple, groups, min_peers: int):
        super().__init__(family, handle, ranks, sections, kernels, params)
        self.groups, self.min_peers = groups, min_peers

    def build(self) -> dict:
        if self._built is None:
            planes, scores, cols = self.handle.records()
            self.handle = _Delivered((planes, scores))
            built = super().build()
            ranks, labels, min_peers = self.ranks, self.groups.labels, self.min_peers
            group = self.groups.group.tolist()
            G, K = len(labels), len(self.kernels)
            floor = np.ascontiguousarray(cols).view(np.float32)[:, :, 0].tolist()
            present = cols[:, :, 1].tolist()
            holder = cols[:, :, 2].view(np.int32).tolist() if cols.size else []
            sc = scores.tolist()

            def referenced(c):
                return {labels[g]: {"value": floor[g][c], "rank": holder[g][c], "ranks": present[g][c]}
                        for g in range(G) if present[g][c] >= min_peers}

            built.update({
                "peer_groups": True,
                "min_peers": min_peers,
                "groups": {labels[g]: self.groups.members(g) for g in range(G)},
                "group_of": {r: labels[group[r]] for r in ranks},
                "unrated_ranks": [r for i, r in enumerate(ranks) if all(x != x for x in sc[i])],
                "section_reference": {name: referenced(K + c) for name, c in self.sections.items()},
                "kernel_reference": {name: referenced(k) for k, name in enumerate(self.kernels)},
            })
            self.groups = None
        return self._built


class _Delivered:
    """Records that are on the host already, behind a handle's ``records()``."""

    __slots__ = ("_rec",)

    def __init__(self, rec):
        self._rec = rec

    def records(self):
        return self._rec


def _copy_scores(d: dict) -> dict:
    """A private copy of a report's follow-up scores (plain dicts, floats, ints and bools all the way down)."""
    return {k: _copy_scores(x) if isinstance(x, dict) else x for k, x in d.items()}


class _RobustSource:
    """What a report keeps of its robust scores: the backend's handle (``records()`` waits for the kernels and copies the
    column records and the scores out on first use), the ranks its rows stand for, the sections it shows with their ids,
    and the kernel names by id as the report's mapper had them at report time."""

    __slots__ = ("handle", "ranks", "sections", "kernels", "min_ranks", "floor", "_built")

    def __init__(self, handle, ranks, sections, kernels, min_ranks: int, floor: float):
        self.handle, self.ranks, self.kernels = handle, tuple(ranks), kernels
        self.min_ranks, self.floor = min_ranks, floor
        self.sections = {n: g for n, g in sections.items() if g is not None}  # (a name whose id is still to be agreed has no column)
        self._built: Optional[dict] = None

    def build(self) -> dict:
        if self._built is None:
            cols, scores = self.handle.records()
            K = len(self.kernels)
            ranks = self.ranks
            f = np.ascontiguousarray(cols).view(np.float32)[:, :3].tolist()
            n = cols[:, 3].tolist()
            sc = scores.tolist()
            with_data = {name: n[k] for k, name in enumerate(self.kernels)}
            with_data.update((name, n[K + g]) for name, g in self.sections.items())
            self._built = {
                "gpu_ratio": {r: sc[i][0][0] for i, r in enumerate(ranks)},
                "gpu_z": {r: sc[i][1][0] for i, r in enumerate(ranks)},
                "section_ratio": {name: {r: sc[i][0][1 + g] for i, r in enumerate(ranks)} for name, g in self.sections.items()},
                "section_z": {name: {r: sc[i][1][1 + g] for i, r in enumerate(ranks)} for name, g in self.sections.items()},
                "section_center": {name: f[K + g][0] for name, g in self.sections.items()},
                "section_spread": {name: f[K + g][2] for name, g in self.sections.items()},
                "kernel_center": {name: f[k][0] for k, name in enumerate(self.kernels)},
                "ranks_with_data": with_data,
                "min_ranks": self.min_ranks,
                "floor": self.floor,
            }
            self.handle = None
        return self._built


def _pace_rank_parts(recs, ranks) -> dict:
    """``{rank: {"gpu": {...}, "sections": {...}}}`` of ``[n_ranks][2][8]`` pace rank records (uint32 bit patterns)."""
    recs = np.ascontiguousarray(recs)
    f, u = recs.view(np.float32).tolist(), recs.tolist()

    def part(i, p):
        columns, slower = u[i][p][2], u[i][p][3]
        d = {"pace": f[i][p][0], "spread": f[i][p][1], "columns": columns, "slower": slower, "faster": u[i][p][4],
             "breadth": slower / columns if columns else None}
        if p == 0:
            d.update(total_us=f[i][p][5], slower_us=f[i][p][6], excess_us=f[i][p][7])
        return d

    return {r: {"gpu": part(i, 0), "sections": part(i, 1)} for i, r in enumerate(ranks)}


class _PaceSource:
    """What a report keeps of its pace scores: the backend's handle (``records()`` waits for the kernels and copies the column
    and rank records out on first use), the ranks its rows stand for, the sections it shows with their ids, the kernel names
    by id as the report's mapper had them at report time, and the parameters in force."""

    __slots__ = ("handle", "ranks", "sections", "kernels", "params", "_built")

    def __init__(self, handle, ranks, sections, kernels, params: dict):
        self.handle, self.ranks, self.kernels, self.params = handle, tuple(ranks), kernels, params
        self.sections = {n: g for n, g in sections.items() if g is not None}  # (a name whose id is still to be agreed has no column)
        self._built: Optional[dict] = None

    def build(self) -> dict:
        if self._built is None:
            cols, recs = self.handle.records()
            K = len(self.kernels)
            center = np.ascontiguousarray(cols).view(np.float32)[:, 0].tolist()
            counts = cols[:, 1:].tolist()

            def column(c):
                return {"center": center[c], "ranks": counts[c][0], "above": counts[c][1], "below": counts[c][2]}

            self._built = {
                "ranks": _pace_rank_parts(recs, self.ranks),
                "kernels": {name: column(k) for k, name in enumerate(self.kernels)},
                "section_columns": {name: column(K + g) for name, g in self.sections.items()},
                "params": dict(self.params),
            }
            self.handle = None
        return self._built


class _PaceGroupSource(_PaceSource):
    """``_PaceSource`` for pace scores per peer group: the handle's column records come per group, and the report also says
    which ranks form which group."""

    __slots__ = ("groups",)

    def __init__(self, handle, ranks, sections, kernels, params: dict, groups):
        super().__init__(handle, ranks, sections, kernels, params)
        self.groups = groups

    def build(self) -> dict:
        if self._built is None:
            cols, recs = self.handle.records()
            rated = _pace_rank_parts(recs, self.ranks)
            K = len(self.kernels)
            labels = self.groups.labels
            group = self.groups.group.tolist()
            G = len(labels)
            center = np.ascontiguousarray(cols).view(np.float32)[:, :, 0].tolist()
            counts = cols[:, :, 1:].tolist()

            def column(c):
                return {labels[g]: {"center": center[g][c], "ranks": counts[g][c][0], "above": counts[g][c][1],
                                    "below": counts[g][c][2]} for g in range(G)}

            self._built = {
                "ranks": rated,
                "kernels": {name: column(k) for k, name in enumerate(self.kernels)},
                "section_columns": {name: column(K + g) for name, g in self.sections.items()},
                "params": dict(self.params),
                "groups": {labels[g]: self.groups.members(g) for g in range(G)},
                "group_of": {r: labels[group[r]] for r in self.ranks},
                "unrated_ranks": [r for r, d in rated.items() if d["gpu"]["columns"] == 0 and d["sections"]["columns"] == 0],
            }
            self.handle = None
        return self._built


def _node_member_rule(d: dict, columns: int, effect: float, breadth: float):
    """``(rated, off_pace)`` of one part of a pace rank record: the pace rule of ``identify_pace_stragglers``."""
    rated = d["columns"] >= columns and d["columns"] > 0
    return rated, bool(rated and d["pace"] <= 1.0 - effect and d["slower"] / d["columns"] >= breadth)


def _node_agreement(t: dict, part: str, label, columns: int, effect: float, breadth: float):
    """``(members_rated, members_off_pace, agree)`` of one node: over its members the report covers, how many have enough
    columns to be rated by the pace rule against the nodes' centre, how many of those are off pace, and the quotient (None
    when the report covers no rated member)."""
    ranks = t["ranks"]
    rule = [_node_member_rule(ranks[r][part], columns, effect, breadth) for r in t["nodes"][label] if r in ranks]
    rated, off = sum(1 for x, _ in rule if x), sum(1 for _, y in rule if y)
    return rated, off, (off / rated if rated else None)


class _NodeSource:
    """What a report keeps of its node scores: the backend's handle (``records()`` waits for the kernels and copies the four
    record blocks out on first use), the ranks its rank rows stand for, the sections it shows with their ids, the kernel names
    by id as the report's mapper had them at report time, the parameters in force and the nodes (a ``backend.PeerGroups``)."""

    __slots__ = ("handle", "ranks", "sections", "kernels", "params", "nodes", "_built")

    def __init__(self, handle, ranks, sections, kernels, params: dict, nodes):
        self.handle, self.ranks, self.kernels, self.params, self.nodes = handle, tuple(ranks), kernels, params, nodes
        self.sections = {n: g for n, g in sections.items() if g is not None}  # (a name whose id is still to be agreed has no column)
        self._built: Optional[dict] = None

    def build(self) -> dict:
        if self._built is None:
            pairs, cols, nrecs, rrecs = self.handle.records()
            K = len(self.kernels)
            labels = self.nodes.labels
            node = self.nodes.group.tolist()
            G = len(labels)
            center = np.ascontiguousarray(cols).view(np.float32)[:, 0].tolist()
            counts = cols[:, 1:].tolist()
            median = np.ascontiguousarray(pairs).view(np.float32)[:, :, 0].tolist()
            present = pairs[:, :, 1].tolist()

            def column(c):
                return {"center": center[c], "nodes": counts[c][0], "above": counts[c][1], "below": counts[c][2],
                        "per_node": {labels[g]: {"median": median[g][c], "ranks": present[g][c]} for g in range(G)}}

            rated = _pace_rank_parts(nrecs, labels)
            for d in rated.values():  # (a node record has no weights: its three sums are empty)
                for key in ("total_us", "slower_us", "excess_us"):
                    del d["gpu"][key]
            t = self._built = {
                "nodes": {labels[g]: self.nodes.members(g) for g in range(G)},
                "node_of": {r: labels[g] for r, g in enumerate(node)},
                "kernels": {name: column(k) for k, name in enumerate(self.kernels)},
                "section_columns": {name: column(K + g) for name, g in self.sections.items()},
                "node_scores": rated,
                "ranks": _pace_rank_parts(rrecs, self.ranks),
                "unrated_nodes": [lab for lab, d in rated.items() if d["gpu"]["columns"] == 0 and d["sections"]["columns"] == 0],
                "params": dict(self.params),
            }
            p = self.params
            for lab, d in rated.items():
                for part in ("gpu", "sections"):
                    d[part]["members_rated"], d[part]["members_off_pace"], d[part]["agree"] = _node_agreement(
                        t, part, lab, p["min_columns"], p["min_effect"], p["min_breadth"])
                for key in ("members_rated", "members_off_pace", "agree"):
                    d[key] = d["gpu"][key]
            self.handle = None
        return self._built


def _peer_spec(peer_groups, what: str = "peer_groups"):
    """``ReportGenerator``'s ``peer_groups`` as the generator keeps it: None (off), ``"auto"`` (inferred per report: work
    groups), a rule (``"block:N"``: label ``rank //
    N``, contiguous stages; ``"mod:N"``: label ``rank % N``) or a tuple of ``int`` / ``str`` labels, one per logical rank.
    Nothing else is accepted.  ``node_groups`` is parsed here too: ``what`` is the option's name in the messages."""
    if peer_groups is None:
        return None
    if isinstance(peer_groups, str) and peer_groups == "auto":
        if what != "peer_groups":
            raise ValueError(f"{what}='auto': only peer_groups are inferred from the table (work groups say which ranks do the "
                             "same work, not which share a host); pass labels, 'block:N' or 'mod:N'")
        return "auto"  # the groups of every report are the work groups inferred from its table (ReportGenerator._peer_for)
    if isinstance(peer_groups, str):
        kind, sep, num = peer_groups.partition(":")
        if kind not in ("block", "mod") or not sep or not num.strip().isdigit():
            raise ValueError(f"{what} must be 'block:N', 'mod:N' or a sequence of labels, got {peer_groups!r}")
        n = int(num)
        if n < 1:
            raise ValueError(f"{what}={peer_groups!r}: N must be at least 1")
        return _backend_mod._PeerRule((kind, n))
    if not isinstance(peer_groups, (list, tuple, np.ndarray)):
        raise TypeError(f"{what} must be 'block:N', 'mod:N' or a list, tuple or ndarray of int or str labels, "
                        f"got {type(peer_groups).__name__}")
    if isinstance(peer_groups, np.ndarray):
        if peer_groups.ndim != 1:
            raise ValueError(f"{what} must have one label per logical rank, got an array of shape {peer_groups.shape}")
        peer_groups = peer_groups.tolist()
    labels = []
    for lab in peer_groups:
        if isinstance(lab, bool) or not isinstance(lab, (int, np.integer, str)):
            raise TypeError(f"{what} labels must be int or str, got {lab!r}")
        labels.append(lab if isinstance(lab, str) else int(lab))
    if not labels:
        raise ValueError(f"{what} must have one label per logical rank, got none")
    return tuple(labels)


def _copy_peer(d):
    """A private copy of a report's peer scores (plain dicts and lists all the way down)."""
    if isinstance(d, dict):
        return {k: _copy_peer(x) for k, x in d.items()}
    return list(d) if isinstance(d, list) else d


class _PeerSource:
    """What a report keeps of its peer-group scores: the backend's handle (``records()`` waits for the kernels and copies the
    column records and the scores out on first use), the ranks its rows stand for, the sections it shows with their ids,
    the kernel names by id as the report's mapper had them at report time, the resolved groups and ``min_ranks``."""

    __slots__ = ("handle", "ranks", "sections", "kernels", "groups", "min_ranks", "_built")

    def __init__(self, handle, ranks, sections, kernels, groups, min_ranks: int):
        self.handle, self.ranks, self.kernels = handle, tuple(ranks), kernels
        self.groups, self.min_ranks = groups, min_ranks
        self.sections = {n: g for n, g in sections.items() if g is not None}  # (a name whose id is still to be agreed has no column)
        self._built: Optional[dict] = None

    def build(self) -> dict:
        if self._built is None:
            cols, scores = self.handle.records()
            K = len(self.kernels)
            ranks, labels, min_ranks = self.ranks, self.groups.labels, self.min_ranks
            group = self.groups.group.tolist()
            G = len(labels)
            floor = np.ascontiguousarray(cols).view(np.float32)[:, :, 0].tolist()
            present = cols[:, :, 1].tolist()
            fastest = cols[:, :, 2].view(np.int32).tolist() if cols.size else []
            sc = scores.tolist()

            def referenced(values, c):
                return {labels[g]: values[g][c] for g in range(G) if present[g][c] >= min_ranks}

            with_data = {name: {labels[g]: present[g][k] for g in range(G)} for k, name in enumerate(self.kernels)}
            with_data.update((name, {labels[g]: present[g][K + c] for g in range(G)}) for name, c in self.sections.items())
            self._built = {
                "groups": {labels[g]: self.groups.members(g) for g in range(G)},
                "group_of": {r: labels[group[r]] for r in ranks},
                "min_ranks": min_ranks,
                "gpu_relative": {r: sc[i][0] for i, r in enumerate(ranks)},
                "section_relative": {name: {r: sc[i][1 + c] for i, r in enumerate(ranks)} for name, c in self.sections.items()},
                "section_floor": {name: referenced(floor, K + c) for name, c in self.sections.items()},
                "section_fastest": {name: referenced(fastest, K + c) for name, c in self.sections.items()},
                "kernel_floor": {name: referenced(floor, k) for k, name in enumerate(self.kernels)},
                "ranks_with_data": with_data,
                "unrated_ranks": [r for i, r in enumerate(ranks) if all(x != x for x in sc[i])],
            }
            self.handle = None
        return self._built


_HISTORY_FAMILIES = ((1, "relative"), (0, "individual"))  # (family word of the record, name) in the order the mappings are listed


class _HistorySource:
    """What a report keeps of the score history as it stood after that report: the backend's handle (``records()`` waits for
    the kernel and copies the records out on first use), the ranks its rows stand for, the sections it shows with their ids,
    which families were computed, and the generator's depth, streak length and thresholds."""

    __slots__ = ("handle", "ranks", "sections", "has_rel", "has_indiv", "capacity", "min_reports", "thresholds", "_built")

    def __init__(self, handle, ranks, sections, has_rel: bool, has_indiv: bool, capacity: int, min_reports: int, thresholds):
        self.handle, self.ranks = handle, tuple(ranks)
        self.sections = {n: g for n, g in sections.items() if g is not None}  # (a name whose id is still to be agreed has no column)
        self.has_rel, self.has_indiv = has_rel, has_indiv
        self.capacity, self.min_reports, self.thresholds = capacity, min_reports, tuple(thresholds)
        self._built: Optional[dict] = None

    def build(self) -> dict:
        if self._built is None:
            rec = np.ascontiguousarray(self.handle.records(), dtype=np.uint32)
            f32 = rec.view(np.float32)[..., :4].tolist()
            u32 = rec[..., 4:].tolist()
            ranks = self.ranks

            def record(i, fam, j):
                f, u = f32[i][fam][j], u32[i][fam][j]
                return {"latest": f[0], "median": f[1], "worst": f[2], "best": f[3], "streak": u[0], "below": u[1],
                        "present": u[2]}

            built: Dict[str, Any] = {"depth": int(rec[0, 0, 0, 7]) if rec.size else 0, "capacity": self.capacity,
                                     "min_reports": self.min_reports, "thresholds": self.thresholds}
            families = self.families()
            for fam, name in families:
                built["gpu_" + name] = {r: record(i, fam, 0) for i, r in enumerate(ranks)}
            for fam, name in families:
                built["section_" + name] = {n: {r: record(i, fam, 1 + g) for i, r in enumerate(ranks)}
                                            for n, g in self.sections.items()}
            self._built = built
            self.handle = None
        return self._built

    def families(self):
        """``(family index of the records, name)`` of the families the report shows, in the order the mappings are listed."""
        return [(fam, name) for fam, name in _HISTORY_FAMILIES if (self.has_rel if fam else self.has_indiv)]


class _PeerHistorySource(_HistorySource):
    """``_HistorySource`` for the peer-score history: the records hold one family, the relative one, and the thresholds are
    ``(gpu, section)``."""

    __slots__ = ()

    def __init__(self, handle, ranks, sections, capacity: int, min_reports: int, thresholds):
        super().__init__(handle, ranks, sections, True, False, capacity, min_reports, thresholds)

    def families(self):
        return [(0, "relative")]


class _TrendSource:
    """What a report keeps of the score trends as they stood after that report: the backend's handle (``records()`` waits for
    the kernel and copies the records out on first use), the ranks its rows stand for, the sections it shows with their ids,
    which families were computed, and the generator's depth, thresholds and rules."""

    __slots__ = ("handle", "ranks", "sections", "has_rel", "has_indiv", "depth", "min_reports", "min_tau", "horizon",
                 "thresholds", "_built")

    def __init__(self, handle, ranks, sections, has_rel: bool, has_indiv: bool, depth: int, min_reports: int, min_tau: float,
                 horizon: int, thresholds):
        self.handle, self.ranks = handle, tuple(ranks)
        self.sections = {n: g for n, g in sections.items() if g is not None}  # (a name whose id is still to be agreed has no column)
        self.has_rel, self.has_indiv = has_rel, has_indiv
        self.depth, self.min_reports, self.min_tau, self.horizon = depth, min_reports, min_tau, horizon
        self.thresholds = tuple(thresholds)
        self._built: Optional[dict] = None

    def build(self) -> dict:
        if self._built is None:
            rec = np.ascontiguousarray(self.handle.records(), dtype=np.uint32)
            f32 = rec.view(np.float32)[..., :2].tolist()
            mk = rec.view(np.int32)[..., 2].tolist()
            usable = rec[..., 3].tolist()
            ranks, min_reports, min_tau = self.ranks, self.min_reports, self.min_tau

            def record(i, fam, j, thr):
                (slope, level), s, p = f32[i][fam][j], mk[i][fam][j], usable[i][fam][j]
                pairs = p * (p - 1) // 2
                tau = s / pairs if pairs else 0.0
                falling = p >= min_reports and slope < 0 and tau <= -min_tau
                if level < thr:
                    left = 0
                elif falling:
                    q = (level - thr) / -slope
                    left = math.ceil(q) if math.isfinite(q) else None  # (a level beyond f32's range crosses nothing)
                else:
                    left = None
                return {"slope": slope, "level": level, "tau": tau, "usable": p, "falling": falling, "reports_left": left}

            built: Dict[str, Any] = {"depth": self.depth, "min_reports": min_reports, "min_tau": min_tau,
                                     "horizon": self.horizon, "thresholds": self.thresholds}
            families = self.families()
            for fam, name, thr, _ in families:
                built["gpu_" + name] = {r: record(i, fam, 0, thr) for i, r in enumerate(ranks)}
            for fam, name, _, thr in families:
                built["section_" + name] = {n: {r: record(i, fam, 1 + g, thr) for i, r in enumerate(ranks)}
                                            for n, g in self.sections.items()}
            self._built = built
            self.handle = None
        return self._built

    def families(self):
        """``(family index of the records, name, GPU threshold, section threshold)`` of the families the report shows."""
        g_rel, s_rel, g_ind, s_ind = self.thresholds
        return [(fam, name, g_rel if fam else g_ind, s_rel if fam else s_ind) for fam, name in _HISTORY_FAMILIES
                if (self.has_rel if fam else self.has_indiv)]


class _PeerTrendSource(_TrendSource):
    """``_TrendSource`` for the peer-score trends: the records hold one family, the relative one, and the thresholds are
    ``(gpu, section)``.  The records and the rule are ``_TrendSource``'s."""

    __slots__ = ()

    def __init__(self, handle, ranks, sections, depth: int, min_reports: int, min_tau: float, horizon: int, thresholds):
        super().__init__(handle, ranks, sections, True, False, depth, min_reports, min_tau, horizon, thresholds)

    def families(self):
        return [(0, "relative") + self.thresholds]


class _SlackSource:
    """What a report keeps of its slack scores: the backend's handle (``records()`` waits for the kernels and copies the
    records out on first use), the ranks its rows stand for, this process' collective keys by column, and the generator's
    rule."""

    __slots__ = ("handle", "ranks", "keys", "min_ranks", "min_share", "max_ratio", "_built")

    def __init__(self, handle, ranks, keys, min_ranks: int, min_share: float, max_ratio: float):
        self.handle, self.ranks, self.keys = handle, tuple(ranks), keys
        self.min_ranks, self.min_share, self.max_ratio = min_ranks, min_share, max_ratio
        self._built: Optional[dict] = None

    def build(self) -> dict:
        if self._built is None:
            job, cols, ranks = (np.ascontiguousarray(a, dtype=np.uint32) for a in self.handle.records())
            typical_waited, typical_share = job[:2].view(np.float32).tolist()
            floors, present = cols[:, 0].copy().view(np.float32).tolist(), cols[:, 1].tolist()
            f = ranks[:, :4].copy().view(np.float32).tolist()
            counts = ranks[:, 4:6].tolist()
            per_rank = {}
            for i, r in enumerate(self.ranks):
                if counts[i][1] == 0:
                    continue  # (no referenced column: this rank has no slack scores)
                coll, waited, comp, share = f[i]
                per_rank[r] = {"collective_us": coll, "waited_us": waited, "compute_us": comp, "share": share,
                               "calls": counts[i][0], "lead_us": typical_waited - waited}
            columns = {c: {"floor_us": floors[c], "ranks": present[c], "kernels": list(self.keys.get(c, ()))}
                       for c in range(SLACK_COLS) if present[c] and not math.isnan(floors[c])}
            self._built = {"ranks": per_rank, "typical_waited_us": typical_waited, "typical_share": typical_share,
                           "ranks_with_data": int(job[2]), "columns": columns, "min_ranks": self.min_ranks,
                           "min_share": self.min_share, "max_ratio": self.max_ratio}
            self.handle = None
        return self._built


class _SlackGroupSource(_SlackSource):
    """What a report keeps of its slack scores per peer group (``ReportGenerator(slack_peer_groups=True)``): ``_SlackSource``
    with the resolved groups and ``min_peers``; the handle's records are per group."""

    __slots__ = ("groups", "min_peers")

    def __init__(self, handle, ranks, keys, groups, min_ranks: int, min_peers: int, min_share: float, max_ratio: float):
        super().__init__(handle, ranks, keys, min_ranks, min_share, max_ratio)
        self.groups, self.min_peers = groups, min_peers

    def build(self) -> dict:
        if self._built is None:
            grp, pairs, ranks = (np.ascontiguousarray(a, dtype=np.uint32) for a in self.handle.records())
            labels, group = self.groups.labels, self.groups.group.tolist()
            G = len(labels)
            typical = grp[:, :2].copy().view(np.float32).tolist()
            floors = pairs[:, :, 0].copy().view(np.float32).tolist()
            present = pairs[:, :, 1].tolist()
            holder = pairs[:, :, 2].copy().view(np.int32).tolist()
            f = ranks[:, :4].copy().view(np.float32).tolist()
            counts = ranks[:, 4:7].tolist()
            per_rank, unrated = {}, []
            for i, r in enumerate(self.ranks):
                if counts[i][1] == 0:
                    if counts[i][2]:
                        unrated.append(r)  # (collective rows, and no pair of its group is referenced: no peers)
                    continue
                coll, waited, comp, share = f[i]
                per_rank[r] = {"collective_us": coll, "waited_us": waited, "compute_us": comp, "share": share,
                               "calls": counts[i][0], "lead_us": typical[group[r]][0] - waited, "group": labels[group[r]]}
            per_group = {}
            for g in range(G):
                columns = {c: {"floor_us": floors[g][c], "ranks": present[g][c], "floor_rank": holder[g][c],
                               "kernels": list(self.keys.get(c, ()))} for c in range(SLACK_COLS) if holder[g][c] >= 0}
                per_group[labels[g]] = {"typical_waited_us": typical[g][0], "typical_share": typical[g][1],
                                        "ranks_with_data": int(grp[g, 2]), "columns": columns}
            self._built = {"ranks": per_rank, "groups": {labels[g]: self.groups.members(g) for g in range(G)},
                           "group_of": {r: labels[group[r]] for r in self.ranks}, "unrated_ranks": unrated,
                           "per_group": per_group, "min_ranks": self.min_ranks, "min_peers": self.min_peers,
                           "min_share": self.min_share, "max_ratio": self.max_ratio, "peer_groups": True}
            self.handle = None
        return self._built


class _WorkSource:
    """What a report keeps of its work groups: the backend's handle (``records()`` waits for the kernels and copies the rank
    records and the job record out on first use), the ranks its rows stand for, the step's parameters and -- where the user
    also passed labels -- the resolved ``peer_groups`` to hold against the inferred ones."""

    __slots__ = ("handle", "ranks", "params", "labelled", "_built")

    def __init__(self, handle, ranks, params: dict, labelled=None):
        self.handle, self.ranks, self.params, self.labelled = handle, tuple(ranks), params, labelled
        self._built: Optional[dict] = None

    def build(self) -> dict:
        if self._built is None:
            rec, job = (np.ascontiguousarray(a, dtype=np.uint32) for a in self.handle.records())
            root = rec[:, 0].copy().view(np.int32).tolist()
            nearest = rec[:, 3].copy().view(np.int32).tolist()
            u = rec.tolist()
            groups: Dict[int, List[int]] = {}
            for r, g in enumerate(root):
                groups.setdefault(g, []).append(r)
            per_rank = {}
            for r in self.ranks:
                _, size, degree, _, n_unlike, n_either, kernels, sections = u[r]
                per_rank[r] = {"size": size, "degree": degree, "loose": degree + 1 < size,
                               "nearest": nearest[r] if nearest[r] >= 0 else None, "nearest_unlike": n_unlike,
                               "nearest_columns": n_either, "kernels": kernels, "sections": sections}
            built = {"groups": groups, "group_of": {r: root[r] for r in self.ranks},
                     "singletons": [g for g, members in groups.items() if len(members) == 1], "ranks": per_rank,
                     "ranks_with_data": int(job[3]), "params": dict(self.params)}
            if self.labelled is not None:
                # the user's groups whose members the table puts into more than one inferred group (host arithmetic)
                conflicts = {}
                for g, label in enumerate(self.labelled.labels):
                    split: Dict[int, List[int]] = {}
                    for r in self.labelled.members(g):
                        split.setdefault(root[r], []).append(r)
                    if len(split) > 1:
                        conflicts[label] = split
                built["label_conflicts"] = conflicts
            self._built = built
            self.handle = self.labelled = None
        return self._built


_LAZY_FIELDS = frozenset((
    "gpu_relative_perf_scores", "section_relative_perf_scores", "gpu_individual_perf_scores",
    "section_individual_perf_scores", "local_section_summaries", "local_kernel_summaries",
))


@dataclasses.dataclass(frozen=True)
class Report:
    """Result of one ``generate_report`` call.

    Two score families, both "current performance / reference performance" in (0, 1]:

    * relative -- reference is the fastest rank's median for the same section / kernel
      (needs the cross-rank exchange);
    * individual -- reference is this rank's own best median so far.

    With ``gather_on_rank0=True`` the score mappings cover every rank and exist on rank 0 only;
    otherwise each rank's report covers just that rank.  Mappings may be empty.

    Fields (same names and order as the reference, reporting.py:73-82):
    ``gpu_relative_perf_scores`` rank -> score; ``section_relative_perf_scores`` section -> rank ->
    score; ``gpu_individual_perf_scores``; ``section_individual_perf_scores``; ``rank_to_node``;
    ``local_section_summaries`` / ``local_kernel_summaries`` this rank's timing statistics;
    ``generate_report_elapsed_time`` [ms]; ``gather_on_rank0``; ``rank``.

    Every mapping is a plain ``dict`` (of plain dicts / floats), as in the reference, so reports can be
    pickled, sent through ``multiprocessing`` queues, deep-copied and ``json.dumps``-ed.  Reports that come
    straight from the device build each mapping on first read (``_from_device``); nothing about that is
    visible from outside except that an unread mapping costs nothing.
    """

    gpu_relative_perf_scores: Mapping[int, float]
    section_relative_perf_scores: Mapping[str, Mapping[int, float]]
    gpu_individual_perf_scores: Mapping[int, float]
    section_individual_perf_scores: Mapping[str, Mapping[int, float]]
    rank_to_node: Mapping[int, str]
    local_section_summaries: Mapping[str, Any]
    local_kernel_summaries: Mapping[str, Any]
    generate_report_elapsed_time: float
    gather_on_rank0: bool
    rank: Optional[int]

    # ---- construction from the device result block -------------------------------------------------
    @classmethod
    def _from_device(cls, source: _ScoreSource, rank_to_node, elapsed_ms: float, gather_on_rank0: bool,
                     rank: Optional[int]) -> "Report":
        self = object.__new__(cls)
        d = self.__dict__
        d["rank_to_node"] = rank_to_node
        d["generate_report_elapsed_time"] = elapsed_ms
        d["gather_on_rank0"] = gather_on_rank0
        d["rank"] = rank
        d["_src"] = source
        return self

    def _flags(self) -> "Optional[_DeviceFlags]":
        """The score kernel's below-threshold bytes (built from the source on first use), or None."""
        d = self.__dict__
        flags = d.get("_device_flags")
        if flags is None:
            src = d.get("_src")
            if src is not None and src.view.thresholds is not None:
                flags = d["_device_flags"] = src.device_flags()
        return flags

    def __getattr__(self, name: str):
        # reached only when normal lookup fails, i.e. for a mapping field that has not been built yet
        if name in _LAZY_FIELDS:
            src = self.__dict__.get("_src")
            if src is not None:
                d = self.__dict__
                value = d[name] = src.build(name, d)
                return value
        raise AttributeError(f"{type(self).__name__!r} object has no attribute {name!r}")

    def _materialise(self) -> None:
        for name in _LAZY_FIELDS:
            getattr(self, name)

    def __getstate__(self):
        """Plain fields only (every mapping built): what pickle / copy / multiprocessing queues carry."""
        self._materialise()
        state = {f.name: self.__dict__[f.name] for f in dataclasses.fields(self)}
        flags = self._flags()
        if flags is not None:
            state["_device_flags"] = flags
        attr = self.__dict__.get("_attr")
        if attr is not None:
            state["_attr"] = attr.build() if isinstance(attr, _AttrSource) else attr  # plain dicts travel
        robust = self.__dict__.get("_robust")
        if robust is not None:
            state["_robust"] = robust.build() if isinstance(robust, _RobustSource) else robust
        peer = self.__dict__.get("_peer")
        if peer is not None:
            state["_peer"] = peer.build() if isinstance(peer, _PeerSource) else peer
        pace = self.__dict__.get("_pace")
        if pace is not None:
            state["_pace"] = pace.build() if isinstance(pace, _PaceSource) else pace
        node = self.__dict__.get("_node")
        if node is not None:
            state["_node"] = node.build() if isinstance(node, _NodeSource) else node
        history = self.__dict__.get("_history")
        if history is not None:
            state["_history"] = history.build() if isinstance(history, _HistorySource) else history
        trends = self.__dict__.get("_trends")
        if trends is not None:
            state["_trends"] = trends.build() if isinstance(trends, _TrendSource) else trends
        for key, source in (("_peer_history", _HistorySource), ("_peer_trends", _TrendSource)):
            held = self.__dict__.get(key)
            if held is not None:
                state[key] = held.build() if isinstance(held, source) else held
        slack = self.__dict__.get("_slack")
        if slack is not None:
            state["_slack"] = slack.build() if isinstance(slack, _SlackSource) else slack
        work = self.__dict__.get("_work")
        if work is not None:
            state["_work"] = work.build() if isinstance(work, _WorkSource) else work
        for fam in row_families.FAMILIES:
            scores = self.__dict__.get(fam.slot)
            if scores is not None:
                state[fam.slot] = scores.build() if isinstance(scores, _RowFamilySource) else scores
        return state

    def __setstate__(self, state) -> None:
        self.__dict__.update(state)

    def explain_gpu_scores(self) -> Dict[str, Dict[int, Dict[str, Any]]]:
        """The kernels behind each rank's GPU score (``ReportGenerator(kernel_attribution=N)``; ``{}`` when the report carries
        no attribution).  A GPU score is the weighted mean of per-kernel scores ``s_k = ref_k / med_k`` with the microseconds
        ``w_k`` spent in kernel k as weights, so its deficit ``1 - score`` splits into per-kernel shares ``w_k * (1 - s_k) / W``.

        ``{"relative": {rank: {"deficit": 1 - score, "explained": sum of the listed shares, "num_kernels": kernels the score
        covers, "kernels": [{"kernel": name, "share", "score": s_k, "lost_us": w_k * (1 - s_k)}, ...]}}, "individual":
        {...}}`` -- the N kernels with the largest ``lost_us``, largest first (ties: the kernel that got its id first);
        families that were not computed are absent; ranks as in the score mappings.  Where the score is NaN the deficit is
        NaN and the list is empty.  Plain dicts, lists, floats and strings.  The first call waits for the attribution
        kernel; ``generate_report`` never does."""
        attr = self.__dict__.get("_attr")
        if attr is None:
            return {}
        if isinstance(attr, _AttrSource):
            attr = self.__dict__["_attr"] = attr.build()
        return _copy_explanation(attr)

    def tail_scores(self) -> Dict[str, Any]:
        """Tail scores (``ReportGenerator(tail_quantile=q)``; ``{}`` when the report carries none).  Every score of a report
        compares medians and cannot see a rank that is slow on SOME iterations; these compare, the same way, the q-quantile
        of every timing row (nearest rank: an actual sample).

        ``{"quantile": q, "gpu_relative": {rank: score}, "section_relative": {section: {rank: score}}, "section_tails":
        {section: {rank: the row's q-quantile, in the row's own unit}}, "kernel_tails": {kernel: {rank: microseconds}}}`` --
        scores are the fastest rank's tail over this rank's (NaN where a rank lacks the row), ranks and sections as in the
        score mappings, rows without samples are left out of the tails.  Plain dicts and floats.  The first call waits for
        the tail kernels and copies their results; ``generate_report`` does not."""
        return self._family_scores("tail")

    def identify_tail_stragglers(self, gpu_rel_threshold: float = 0.75, section_rel_threshold: float = 0.75) -> Dict[str, Any]:
        """Ranks whose TAIL scores fall strictly below the thresholds (NaN is never flagged): ``{'straggler_gpus_relative':
        set[StragglerId], 'straggler_sections_relative': {section: set}}``; a section appears only if somebody is flagged
        for it.  Empty sets when the report carries no tail scores."""
        return self._identify_relative(self.tail_scores(), gpu_rel_threshold, section_rel_threshold)

    def onset_scores(self) -> Dict[str, Any]:
        """Onset scores (``ReportGenerator(onset_detection=True)``; ``{}`` when the report carries none).  Medians, tails and
        robust scores are order statistics; these look at the ORDER of a window's samples: per timing row the single split of
        the time axis that explains most of the row's variance by one step (least squares), the means either side of it and
        the share of the variance it explains.

        ``{"gpu_relative": {rank: score}, "section_relative": {section: {rank: score}}, "section_onsets": {section: {rank:
        {"shift", "before", "after", "strength", "samples_ago", "window"}}}, "kernel_onsets": {kernel: {rank: {...}}},
        "min_segment": x, "min_strength": x}`` -- ``shift`` is ``after / before`` where the step is a slow-down that explains
        at least ``min_strength`` of the row's variance, 1.0 otherwise; ``samples_ago`` of the row's ``window`` samples lie
        behind the step; scores are the steadiest rank's shift over this rank's (NaN where a rank lacks the row): 1 = shifted
        no more than the steadiest rank, so a phase change of the whole job flags nobody.  Ranks and sections as in the score
        mappings, rows without samples are left out of the onsets.  Plain dicts and floats.  The first call waits for the
        onset kernels and copies their results; ``generate_report`` does not."""
        return self._family_scores("onset")

    def identify_onset_stragglers(self, gpu_rel_threshold: float = 0.75, section_rel_threshold: float = 0.75) -> Dict[str, Any]:
        """Ranks whose ONSET scores fall strictly below the thresholds (NaN is never flagged): ``{'straggler_gpus_relative':
        set[StragglerId], 'straggler_sections_relative': {section: set}}``; a section appears only if somebody is flagged
        for it.  Empty sets when the report carries no onset scores."""
        return self._identify_relative(self.onset_scores(), gpu_rel_threshold, section_rel_threshold)

    def period_scores(self) -> Dict[str, Any]:
        """Period scores (``ReportGenerator(period_detection=True)``; ``{}`` when the report carries none).  Whether a rank is
        slow ON A BEAT -- a stall every P-th sample, which moves no median and no quantile and is no step: per timing row the
        samples, in time order, are folded over every period up to ``max_period`` (and a quarter of the row), and the
        smallest period whose phase means explain (adjusted R^2) at least 0.95 of what the best period explains is kept.

        ``{"gpu_relative": {rank: score}, "section_relative": {section: {rank: score}}, "section_periods": {section: {rank:
        {"period", "samples_ago", "peak", "rest", "excess", "strength", "window"}}}, "kernel_periods": {kernel: {rank:
        {...}}}, "max_period": P, "min_strength": x}`` -- ``period`` is counted in samples of that row (0: none found), the
        slow phase last occurred ``samples_ago`` samples before the end of the row's ``window`` samples, ``peak`` is the mean of
        the slow phase and ``rest`` that of all others, ``excess`` is ``peak / rest`` where the beat explains at least
        ``min_strength`` of the row's variance, 1.0 otherwise; scores are the steadiest rank's excess over this rank's (NaN
        where a rank lacks the row): 1 = stalls no more than the steadiest rank, so a beat of the whole job flags nobody.
        Ranks and sections as in the score mappings, rows without samples are left out.  Plain dicts and floats.  The first
        call waits for the period kernels and copies their results; ``generate_report`` does not."""
        return self._family_scores("period")

    def identify_period_stragglers(self, gpu_rel_threshold: float = 0.75, section_rel_threshold: float = 0.75) -> Dict[str, Any]:
        """Ranks whose PERIOD scores fall strictly below the thresholds (NaN is never flagged): ``{'straggler_gpus_relative':
        set[StragglerId], 'straggler_sections_relative': {section: set}}``; a section appears only if somebody is flagged
        for it.  Empty sets when the report carries no period scores."""
        return self._identify_relative(self.period_scores(), gpu_rel_threshold, section_rel_threshold)

    def episode_scores(self) -> Dict[str, Any]:
        """Episode scores (``ReportGenerator(episode_detection=True)``; ``{}`` when the report carries none).  Whether a rank
        was slow FOR ONE STRETCH of the window and then recovered -- which moves no median, is below what a quantile looks at
        when it is short, is no step and no beat: per timing row the interval ``[a, b)`` of its samples, in time order, that
        spent most time above the row's mean, with at least ``min_length`` of the row (never fewer than 8 samples) inside and
        either side of it.

        ``{"gpu_scores": {rank: score}, "section_scores": {section: {rank: score}}, "section_episodes": {section: {rank:
        {"length", "samples_ago", "began_ago", "window", "inside", "outside", "strength", "excess", "open_ended"}}},
        "kernel_episodes": {kernel: {rank: {...}}}, "min_length": f, "min_strength": x}`` (``gpu_relative`` and
        ``section_relative`` name the two score mappings as well) -- the episode lasted ``length`` samples of that row (0:
        none found), ended ``samples_ago`` and began ``began_ago`` samples before the end of the row's ``window`` samples;
        ``inside`` is its mean and ``outside`` that of all other samples, ``strength`` the share of the row's variance the
        two-level pulse explains, ``excess`` is ``inside / outside`` where the strength is at least ``min_strength``, 1.0
        otherwise; ``open_ended`` says that the stretch runs to the last sample an episode may end at: the row stepped up and
        has not recovered, and ``onset_scores()`` is the better reading.  Scores are the steadiest rank's excess over this
        rank's (NaN where a rank lacks the row): 1 = no stretch slower than the steadiest rank's, so a stretch the whole job
        shares flags nobody.  Ranks and sections as in the score mappings, rows without samples are left out.  Plain dicts
        and floats.  The first call waits for the episode kernels and copies their results; ``generate_report`` does not."""
        return self._family_scores("episode")

    def identify_episode_stragglers(self, gpu_rel_threshold: float = 0.75, section_rel_threshold: float = 0.75) -> Dict[str, Any]:
        """Ranks whose EPISODE scores fall strictly below the thresholds (NaN is never flagged): ``{'straggler_gpus_relative':
        set[StragglerId], 'straggler_sections_relative': {section: set}}``; a section appears only if somebody is flagged
        for it.  Empty sets when the report carries no episode scores."""
        return self._identify_relative(self.episode_scores(), gpu_rel_threshold, section_rel_threshold)

    def robust_scores(self) -> Dict[str, Any]:
        """Robust scores (``ReportGenerator(robust_scores=True)``; ``{}`` when the report carries none).  Every relative score
        of a report divides the FASTEST rank's median by this rank's; these rate a rank against the job's own middle and
        spread instead: per section and kernel the lower median ``ctr`` of the ranks that have the row, the median absolute
        deviation ``mad`` around it, ``scale = max(1.4826 * mad, floor * ctr)``.

        ``{"gpu_ratio": {rank: x}, "gpu_z": {rank: x}, "section_ratio": {section: {rank: ctr / median}}, "section_z":
        {section: {rank: (median - ctr) / scale}}, "section_center": {section: ctr}, "section_spread": {section: scale},
        "kernel_center": {kernel: microseconds}, "ranks_with_data": {section or kernel: ranks that have the row}, "min_ranks":
        n, "floor": x}`` -- a ratio above 1 is faster than the median, a positive z slower; the GPU entries are the means of
        the per-kernel ratios and z weighted by the microseconds spent in each kernel; NaN where a rank lacks the row or
        fewer than ``min_ranks`` ranks have it.  Ranks and sections as in the score mappings.  Plain dicts and floats.  The
        first call waits for the robust kernels and copies their results; ``generate_report`` does not."""
        robust = self.__dict__.get("_robust")
        if robust is None:
            return {}
        if isinstance(robust, _RobustSource):
            robust = self.__dict__["_robust"] = robust.build()
        return _copy_scores(robust)

    def identify_robust_stragglers(self, gpu_z_threshold: float = 3.5, section_z_threshold: float = 3.5) -> Dict[str, Any]:
        """Ranks whose robust z-scores lie strictly ABOVE the thresholds (NaN is never flagged): ``{'straggler_gpus_relative':
        set[StragglerId], 'straggler_sections_relative': {section: set}}``; a section appears only if somebody is flagged
        for it.  3.5 is the conventional cut-off for modified z-scores (Iglewicz and Hoaglin): a default, not a measurement.
        Empty sets when the report carries no robust scores."""
        t = self.robust_scores()
        gr = [r for r, z in t.get("gpu_z", {}).items() if z > gpu_z_threshold]
        sr = {n: [r for r, z in v.items() if z > section_z_threshold] for n, v in t.get("section_z", {}).items()}
        return {"straggler_gpus_relative": self._ids(gr),
                "straggler_sections_relative": {n: self._ids(r) for n, r in sr.items() if r}}

    def peer_scores(self) -> Dict[str, Any]:
        """Peer-group scores (``ReportGenerator(peer_groups=...)``; ``{}`` when the report carries none).  Every relative score
        of a report divides the median of the fastest rank OF THE WHOLE JOB by this rank's; these take the fastest rank of the
        rank's own group -- the ranks doing the same work: a pipeline stage, an expert group, a role -- as the reference.

        ``{"groups": {label: [ranks]}`` (every logical rank of the job), ``"group_of": {rank: label}`` (this report's ranks),
        ``"min_ranks": n, "gpu_relative": {rank: x}, "section_relative": {section: {rank: floor / median}}, "section_floor":
        {section: {label: microseconds}}, "section_fastest": {section: {label: rank}}, "kernel_floor": {kernel: {label:
        microseconds}}, "ranks_with_data": {section or kernel: {label: ranks of the group that have the row}},
        "unrated_ranks": [ranks whose every score is NaN]}`` -- the GPU entries are the means of the per-kernel quotients
        weighted by the microseconds spent in each kernel; NaN where a rank lacks the row or fewer than ``min_ranks`` ranks of
        its group have it (a group appears under a floor only where it has one); a rank alone in its group has no peer and is
        unrated at the default ``min_ranks`` of 2.  Plain dicts, lists, floats and ints.  The first call waits for the peer
        kernels and copies their results; ``generate_report`` does not."""
        peer = self.__dict__.get("_peer")
        if peer is None:
            return {}
        if isinstance(peer, _PeerSource):
            peer = self.__dict__["_peer"] = peer.build()
        return _copy_peer(peer)

    def identify_peer_stragglers(self, gpu_rel_threshold: float = 0.75, section_rel_threshold: float = 0.75) -> Dict[str, Any]:
        """Ranks whose PEER-GROUP scores fall strictly below the thresholds (NaN is never flagged): ``{'straggler_gpus_relative':
        set[StragglerId], 'straggler_sections_relative': {section: set}}``; a section appears only if somebody is flagged
        for it.  Empty sets when the report carries no peer scores."""
        return self._identify_relative(self.peer_scores(), gpu_rel_threshold, section_rel_threshold)

    def pace_scores(self) -> Dict[str, Any]:
        """Pace scores (``ReportGenerator(pace_scores=True)``; ``{}`` when the report carries none).  Every other score asks
        whether some row of a rank is MUCH slower than a reference; these ask whether a rank is a LITTLE slower in nearly all of
        its kernels -- a card held a clock step down, a throttling HBM stack, a marginal power rail.  Per kernel and section
        the reference is the job's lower median; a rank's ``pace`` is the lower median, across its columns, of median / own
        (above 1: faster than the job's median), ``spread`` the median absolute deviation of those quotients around it.

        ``{"ranks": {rank: {"gpu": {...}, "sections": {...}}}, "kernels": {kernel: {...}}, "section_columns": {section: {...}},
        "params": {"min_ranks", "min_columns", "min_effect", "min_breadth"}}`` -- a rank's ``gpu`` (its kernel columns) and
        ``sections`` parts hold ``pace``, ``spread``, ``columns`` (those where the rank has data and at least ``min_ranks``
        ranks do), ``slower`` / ``faster`` (columns where it is above / below the job's median), ``breadth`` (``slower /
        columns``, None at 0) and, for ``gpu``, ``total_us``, ``slower_us`` (microseconds in all / in the slower columns) and
        ``excess_us`` (microseconds spent above the job's median pace in the window, signed).  A kernel or section holds the
        column's ``center`` (NaN where fewer than ``min_ranks`` ranks have it), ``ranks`` with data and how many of them are
        ``above`` / ``below`` the center.  NaN where a part has no column.  Plain dicts, floats and ints.  The first call waits
        for the pace kernels and copies their results; ``generate_report`` does not.

        With ``ReportGenerator(pace_peer_groups=True)`` the reference of a column is the lower median of the rank's OWN peer
        group, and "the job's median" above reads "its group's median".  ``"ranks"`` keeps its shape; ``"params"`` gains
        ``"min_peers"`` and ``"peer_groups": True``; a kernel or section maps each group's label to its ``{"center", "ranks",
        "above", "below"}``; and ``"groups"``, ``"group_of"`` and ``"unrated_ranks"`` (ranks without a column in either
        part: alone in their group, say) are spelled as in ``peer_scores()``.  A pair of group and column is a reference
        when at least ``max(min_peers, min(min_ranks, the group's size))`` of the group's ranks have it."""
        pace = self.__dict__.get("_pace")
        if pace is None:
            return {}
        if isinstance(pace, _PaceSource):
            pace = self.__dict__["_pace"] = pace.build()
        if pace["params"].get("peer_groups"):
            return _copy_peer(pace)  # (the groups' member lists are copied too)
        return _copy_scores(pace)

    def identify_pace_stragglers(self, min_effect: Optional[float] = None, min_breadth: Optional[float] = None,
                                 min_columns: Optional[int] = None) -> Dict[str, Any]:
        """Ranks that are a little slower in nearly everything: a part of a rank (its kernels, its sections) is named iff it
        has at least ``min_columns`` columns, its ``pace`` is at most ``1 - min_effect`` and it is slower than the job's median
        in at least ``min_breadth`` of them (NaN never names).  Both an effect size and breadth: a healthy rank whose silicon
        is 1 % slow is also slower in nearly every kernel.  ``{'straggler_gpus_relative': set[StragglerId],
        'straggler_section_ranks_relative': set[StragglerId]}``; the defaults are the generator's (8, 0.03 and 0.9 unless
        told otherwise: defaults, not measurements).  Empty sets when the report carries no pace scores."""
        t = self.pace_scores()
        if not t:
            return {"straggler_gpus_relative": set(), "straggler_section_ranks_relative": set()}
        params = t["params"]
        effect = params["min_effect"] if min_effect is None else min_effect
        breadth = params["min_breadth"] if min_breadth is None else min_breadth
        columns = params["min_columns"] if min_columns is None else min_columns

        def named(part):
            return [r for r, d in t["ranks"].items()
                    if d[part]["columns"] >= columns and d[part]["columns"] > 0 and d[part]["pace"] <= 1.0 - effect
                    and d[part]["slower"] / d[part]["columns"] >= breadth]

        return {"straggler_gpus_relative": self._ids(named("gpu")),
                "straggler_section_ranks_relative": self._ids(named("sections"))}

    def node_scores(self) -> Dict[str, Any]:
        """Node scores (``ReportGenerator(node_scores=True)``; ``{}`` when the report carries none): the pace scores one level
        up.  A fault of the HOST -- failed fans, a capped PSU, a throttling CPU, the wrong power profile -- makes every GPU of
        one node a few per cent slower in everything; the pace scores then name all of its ranks and cannot say that they are
        one incident.  Here a node's value of a kernel or section is the lower median of its ranks, the reference of a column
        is the lower median of the NODES' values (one node, one vote), and a node's ``pace`` is the lower median across its
        columns of reference / own.  The centre is the job's: a lockstep model, as for the job-wide pace scores.

        ``{"nodes": {label: [ranks]}, "node_of": {rank: label}, "kernels": {kernel: {...}}, "section_columns": {section:
        {...}}, "node_scores": {label: {...}}, "ranks": {rank: {...}}, "unrated_nodes": [labels], "params": {...}}``.  A kernel
        or section holds ``center`` (NaN where fewer than ``min_nodes`` nodes have a value), ``nodes`` with a value, how many
        of them are ``above`` / ``below`` it, and ``per_node``: label -> ``{"median", "ranks"}`` (NaN where fewer than
        ``max(1, min(min_members, the node's size))`` of its ranks have data).  A node holds ``gpu`` and ``sections`` parts with
        ``pace``, ``spread``, ``columns``, ``slower``, ``faster`` and ``breadth`` as ``pace_scores()`` spells a rank's, plus
        ``members_rated`` (its ranks THIS REPORT COVERS that have at least ``min_columns`` columns), ``members_off_pace``
        (those of them the pace rule names against the nodes' centre) and ``agree`` (their quotient; None where no member is
        rated); the three of the ``gpu`` part are repeated at the node's top level.  A report that covers one rank only
        (``gather_on_rank0=False``) still holds every node's record, with ``agree`` over what it sees.  ``ranks`` holds every
        reported rank's record against the nodes' centre, spelled as in ``pace_scores()``: ``excess_us`` is the microseconds
        above the pace of the job's nodes.  ``unrated_nodes``: nodes without a column in either part.  Plain dicts, lists,
        floats and ints.  The first call waits for the node kernels and copies their results; ``generate_report`` does not."""
        node = self.__dict__.get("_node")
        if node is None:
            return {}
        if isinstance(node, _NodeSource):
            node = self.__dict__["_node"] = node.build()
        return _copy_peer(node)  # (the nodes' member lists are copied too)

    def identify_node_stragglers(self, min_effect: Optional[float] = None, min_breadth: Optional[float] = None,
                                 min_columns: Optional[int] = None, min_agree: Optional[float] = None) -> Dict[str, Any]:
        """Nodes that are a little slower in nearly everything: a part of a node (its kernels, its sections) is named iff it has
        at least ``min_columns`` columns, its ``pace`` is at most ``1 - min_effect``, it is slower than the nodes' centre in at
        least ``min_breadth`` of them, and at least ``min_agree`` of its rated members that the report covers are themselves
        off pace by the pace rule against the same centre (a node none of whose rated members the report covers is not
        named).  ``{'straggler_nodes': set of labels, 'straggler_section_nodes': set of labels, 'ranks_off_pace_alone':
        set[StragglerId], 'section_ranks_off_pace_alone': set[StragglerId]}`` -- the last two are the ranks off pace whose
        node is not named: a slow GPU, not a slow host.  The defaults are the generator's (8, 0.03, 0.9 and 0.75 unless
        told otherwise: defaults, not measurements).  Empty sets when the report carries no node scores."""
        t = self.node_scores()
        if not t:
            return {"straggler_nodes": set(), "straggler_section_nodes": set(), "ranks_off_pace_alone": set(),
                    "section_ranks_off_pace_alone": set()}
        params = t["params"]
        effect = params["min_effect"] if min_effect is None else min_effect
        breadth = params["min_breadth"] if min_breadth is None else min_breadth
        columns = params["min_columns"] if min_columns is None else min_columns
        agree = params["min_agree"] if min_agree is None else min_agree

        def named(part):
            nodes = set()
            for lab, d in t["node_scores"].items():
                if not _node_member_rule(d[part], columns, effect, breadth)[1]:
                    continue
                share = _node_agreement(t, part, lab, columns, effect, breadth)[2]
                if share is not None and share >= agree:
                    nodes.add(lab)
            alone = [r for r, d in t["ranks"].items()
                     if _node_member_rule(d[part], columns, effect, breadth)[1] and t["node_of"][r] not in nodes]
            return nodes, self._ids(alone)

        gpu, sections = named("gpu"), named("sections")
        return {"straggler_nodes": gpu[0], "straggler_section_nodes": sections[0], "ranks_off_pace_alone": gpu[1],
                "section_ranks_off_pace_alone": sections[1]}

    def score_history(self) -> Dict[str, Any]:
        """The score history as it stood after this report (``ReportGenerator(score_history=H)``; ``{}`` when the report
        carries none).  Every other score looks inside one report window; this looks ACROSS reports: per rank and score, what
        the last ``H`` reports of the generator said.

        ``{"depth": reports the history holds (at most H), "capacity": H, "min_reports": M, "thresholds": (gpu_rel,
        section_rel, gpu_indiv, section_indiv), "gpu_relative": {rank: rec}, "gpu_individual": {rank: rec},
        "section_relative": {section: {rank: rec}}, "section_individual": {...}}`` with ``rec = {"latest": this report's
        score, "median": the lower median of the scores present, "worst", "best", "streak": how many of the newest reports in
        a row were below the threshold (0 when this one was not; a report without the score ends it), "below": reports below
        the threshold, "present": reports that had the score at all}`` -- all actual scores, NaN where no report had one.
        Families that were not computed are left out; ranks and sections as in the score mappings.  Plain dicts, floats and
        ints.  The first call waits for the history kernel and copies its records; ``generate_report`` does not."""
        history = self.__dict__.get("_history")
        if history is None:
            return {}
        if isinstance(history, _HistorySource):
            history = self.__dict__["_history"] = history.build()
        return _copy_scores(history)

    def identify_persistent_stragglers(self, min_reports: Optional[int] = None) -> Dict[str, Any]:
        """Ranks whose score has been below its threshold for the last ``min_reports`` reports IN A ROW, this one included
        (default: the generator's ``persistence_min_reports``): the four keys of ``identify_stragglers``, ``StragglerId``
        sets; a section appears only if somebody is flagged for it.  One slow window flags nobody here.  Empty sets when
        the report carries no score history."""
        return self._identify_persistent(self.score_history(), min_reports)

    def _identify_persistent(self, t, min_reports) -> Dict[str, Any]:
        """The streak rule on a history ``t`` (``score_history()`` or ``peer_history()``): the four keys."""
        m = t.get("min_reports", 1) if min_reports is None else min_reports
        if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or m < 1:
            raise ValueError(f"min_reports must be an integer >= 1, got {min_reports!r}")

        def gpus(key):
            return self._ids([r for r, rec in t.get(key, {}).items() if rec["streak"] >= m])

        def sections(key):
            flagged = {n: [r for r, rec in v.items() if rec["streak"] >= m] for n, v in t.get(key, {}).items()}
            return {n: self._ids(r) for n, r in flagged.items() if r}

        return {"straggler_gpus_relative": gpus("gpu_relative"), "straggler_gpus_individual": gpus("gpu_individual"),
                "straggler_sections_relative": sections("section_relative"),
                "straggler_sections_individual": sections("section_individual")}

    def score_trends(self) -> Dict[str, Any]:
        """Whether each score is FALLING from report to report, as the score history stood after this report
        (``ReportGenerator(score_history=H, score_trends=True)``; ``{}`` when the report carries none).  The history says for
        how many reports a score has been below its threshold; this says that a score is on its way there, and when it
        arrives.

        ``{"depth": reports the history holds (at most H), "min_reports", "min_tau", "horizon", "thresholds": (gpu_rel,
        section_rel, gpu_indiv, section_indiv), "gpu_relative": {rank: rec}, "gpu_individual": {rank: rec},
        "section_relative": {section: {rank: rec}}, "section_individual": {...}}`` with ``rec = {"slope": the Theil-Sen slope
        -- the lower median of the slopes of all pairs of usable (finite) scores, the change per report, negative when the
        score falls; NaN with fewer than two --, "level": the trend line's value at this report, "tau": Kendall's tau, the
        Mann-Kendall statistic over the number of pairs, in [-1, 1] (0.0 without a pair), "usable": scores the estimate rests
        on, "falling": usable >= min_reports and slope < 0 and tau <= -min_tau, "reports_left": 0 where the level is already
        below the threshold, else -- when falling -- the reports until the trend line crosses it,
        ceil((level - threshold) / -slope), else None}``.  One bad window barely moves slope or level: both are medians.
        Families that were not computed are left out; ranks and sections as in the score mappings.  Plain dicts, floats, ints
        and bools.  The first call waits for the trend kernel and copies its records; ``generate_report`` does not."""
        trends = self.__dict__.get("_trends")
        if trends is None:
            return {}
        if isinstance(trends, _TrendSource):
            trends = self.__dict__["_trends"] = trends.build()
        return _copy_scores(trends)

    def identify_declining_stragglers(self, horizon: Optional[int] = None) -> Dict[str, Any]:
        """Ranks whose score is falling and whose trend line crosses the threshold within ``horizon`` reports (default: the
        generator's ``trend_horizon``) -- ``falling`` and ``reports_left <= horizon`` in ``score_trends()``: the four keys of
        ``identify_stragglers``, ``StragglerId`` sets; a section appears only if somebody is flagged for it.  A warning, ahead
        of ``identify_stragglers``: a rank named here may still be above its threshold.  Empty sets when the report carries
        no score trends."""
        return self._identify_declining(self.score_trends(), horizon)

    def _identify_declining(self, t, horizon) -> Dict[str, Any]:
        """The horizon rule on trends ``t`` (``score_trends()`` or ``peer_trends()``): the four keys."""
        h = t.get("horizon", 0) if horizon is None else horizon
        if isinstance(h, bool) or not isinstance(h, (int, np.integer)) or h < 0:
            raise ValueError(f"horizon must be an integer >= 0, got {horizon!r}")

        def hit(rec):
            return rec["falling"] and rec["reports_left"] is not None and rec["reports_left"] <= h

        def gpus(key):
            return self._ids([r for r, rec in t.get(key, {}).items() if hit(rec)])

        def sections(key):
            flagged = {n: [r for r, rec in v.items() if hit(rec)] for n, v in t.get(key, {}).items()}
            return {n: self._ids(r) for n, r in flagged.items() if r}

        return {"straggler_gpus_relative": gpus("gpu_relative"), "straggler_gpus_individual": gpus("gpu_individual"),
                "straggler_sections_relative": sections("section_relative"),
                "straggler_sections_individual": sections("section_individual")}

    def _held(self, key: str, source) -> Dict[str, Any]:
        held = self.__dict__.get(key)
        if held is None:
            return {}
        if isinstance(held, source):
            held = self.__dict__[key] = held.build()
        return _copy_scores(held)

    def peer_history(self) -> Dict[str, Any]:
        """The history of the PEER scores as it stood after this report (``ReportGenerator(peer_groups=..., peer_history=H)``;
        ``{}`` when the report carries none): ``score_history()`` for ``peer_scores()``.  In a job whose ranks legitimately
        differ the job-wide history rates every rank of a slower stage low in every report; this one looks, across reports,
        at each rank against the ranks doing the same work.

        ``{"depth", "capacity": H, "min_reports": M, "thresholds": (gpu, section), "gpu_relative": {rank: rec},
        "section_relative": {section: {rank: rec}}}`` with ``rec`` as ``score_history()`` spells it.  A report in which a rank
        was unrated (alone in its group, a section its group has no reference for) is a report without the score: it ends the
        streak.  The history is per rank, whatever the rank's group was in each report: it does not notice that a rank's
        peers changed between reports (``peer_groups="auto"``).  The first call waits for the kernel and copies its records;
        ``generate_report`` does not."""
        return self._held("_peer_history", _HistorySource)

    def identify_persistent_peer_stragglers(self, min_reports: Optional[int] = None) -> Dict[str, Any]:
        """Ranks whose PEER score has been strictly below its threshold for the last ``min_reports`` reports IN A ROW, this
        one included (default: the generator's ``peer_persistence_min_reports``): the two keys of
        ``identify_peer_stragglers``.  Empty sets when the report carries no peer history."""
        out = self._identify_persistent(self.peer_history(), min_reports)
        return {key: out[key] for key in ("straggler_gpus_relative", "straggler_sections_relative")}

    def peer_trends(self) -> Dict[str, Any]:
        """Whether each PEER score is falling from report to report (``ReportGenerator(peer_history=H, peer_trends=True)``;
        ``{}`` when the report carries none): ``score_trends()`` for the peer history, with ``"thresholds": (gpu, section)``
        and the relative family only.  Records and rule are those of ``score_trends()``."""
        return self._held("_peer_trends", _TrendSource)

    def identify_declining_peer_stragglers(self, horizon: Optional[int] = None) -> Dict[str, Any]:
        """Ranks whose PEER score is falling and whose trend line crosses the threshold within ``horizon`` reports (default:
        the generator's ``trend_horizon``, else ``peer_history``): the two keys of ``identify_peer_stragglers``.  Empty sets
        when the report carries no peer trends."""
        out = self._identify_declining(self.peer_trends(), horizon)
        return {key: out[key] for key in ("straggler_gpus_relative", "straggler_sections_relative")}

    def slack_scores(self) -> Dict[str, Any]:
        """Whom the job WAITS FOR in collectives (``ReportGenerator(collective_slack=True)``; ``{}`` when the report carries
        none).  A rank whose host is slow launches late, computes at the usual speed and ends its sections in a collective like
        everybody else: every other score reads 1.  Inside the collective kernels the late rank spends only the transfer time,
        every other rank that plus the wait for it.

        ``{"ranks": {rank: {"collective_us": time in collective kernels this window, "waited_us": the part of it above the
        job's floor -- per column (collective kernel) calls x (this rank's mean per call - the smallest mean of any rank) --,
        "compute_us": time in the other kernels, "share": waited_us / (collective_us + compute_us), "calls", "lead_us":
        typical_waited_us - waited_us, what the others wait for this rank}}, "typical_waited_us", "typical_share": the lower
        medians over the ranks with data, "ranks_with_data", "columns": {column: {"floor_us", "ranks": ranks present,
        "kernels": this process' collective kernels in it}}, "min_ranks", "min_share", "max_ratio"}``.  Only columns that at
        least ``min_ranks`` ranks have are used; a rank without one is left out.  Per-kernel timing only: without collective
        rows (region timing) the result is empty.  Plain dicts, floats and ints.  The first call waits for the kernels and
        copies their records; ``generate_report`` does not.

        With ``ReportGenerator(slack_peer_groups=True)`` the floor of a column is the smallest mean among the rank's OWN peer
        group (``peer_groups``) and the typical wait is its group's: ``"ranks"`` holds the same record per rank plus
        ``"group"`` (the label), ``lead_us`` being taken against the group's typical wait; ``"groups"``, ``"group_of"`` and
        ``"unrated_ranks"`` as ``peer_scores()`` spells them (unrated: ranks with collective rows none of which enough peers
        have); ``"per_group": {label: {"typical_waited_us", "typical_share", "ranks_with_data", "columns": {column:
        {"floor_us", "ranks", "floor_rank", "kernels"}}}}``; ``"min_ranks"``, ``"min_peers"``, ``"min_share"``,
        ``"max_ratio"`` and ``"peer_groups": True``.  There is no job-wide typical wait then."""
        slack = self.__dict__.get("_slack")
        if slack is None:
            return {}
        if isinstance(slack, _SlackSource):
            slack = self.__dict__["_slack"] = slack.build()
        return _copy_peer(slack) if slack.get("peer_groups") else _copy_scores(slack)

    def work_groups(self) -> Dict[str, Any]:
        """Which ranks do the SAME WORK, inferred from the report's table (``ReportGenerator(work_groups=True)`` or
        ``peer_groups="auto"``; ``{}`` when the report carries none).  The signature of a rank's work is which kernel ids and
        section ids it has at all and how often each kernel ran in the window (its weight over its median): a slow GPU changes
        neither, so a straggler stays in the group of its peers.  Two ranks are alike when at most ``max_unlike`` of the columns
        either of them has differ -- present on one only, or call counts more than ``1 + count_tol`` apart -- and the groups
        are the connected components of that relation, named by their lowest rank.

        ``{"groups": {root: [ranks]}`` (every rank of the job), ``"group_of": {rank: root}``, ``"singletons": [roots of groups of
        one rank]``, ``"ranks": {rank: {"size", "degree" (alike ranks), "loose" (degree + 1 < size: the group is a chain, not a
        clique -- single linkage joined ranks that are not alike each other), "nearest" (the other rank with the smallest share
        of differing columns, the lower rank on a tie; None where no other rank has data), "nearest_unlike", "nearest_columns",
        "kernels", "sections" (present columns)}}, "ranks_with_data", "params": {"count_tol", "max_unlike", "max_unlike_ppm"}}``;
        with explicit ``peer_groups`` also ``"label_conflicts": {label: {root: [members]}}`` -- the user's groups whose members
        fall into more than one inferred group.  ``group_of`` and ``ranks`` cover the ranks of the score mappings.  In
        region-stamp timing mode a rank has few columns and equal presence gives one group; call counts saturate at the ring
        capacity.  Plain dicts, lists, ints and floats.  The first call waits for the kernels; ``generate_report`` never does
        (``peer_groups="auto"`` does: the peer step needs the groups)."""
        work = self.__dict__.get("_work")
        if work is None:
            return {}
        if isinstance(work, _WorkSource):
            work = self.__dict__["_work"] = work.build()
        return _copy_peer(work)  # (nested dicts and lists, as the peer scores)

    def identify_slack_stragglers(self, min_share: Optional[float] = None, max_ratio: Optional[float] = None) -> Dict[str, Any]:
        """Ranks the others wait for: ``{"straggler_gpus_slack": set[StragglerId]}``.  A rank with data is named iff the job
        as a whole waits (``typical_share >= min_share``, default the generator's 0.05, and ``typical_waited_us > 0``) and
        this rank hardly does (``waited_us <= max_ratio * typical_waited_us``, default 0.25).  If half the ranks or more are
        late the typical wait is about 0 and nobody is named.  0.05 and 0.25 are defaults, not measurements.  An empty set
        when the report carries no slack scores.

        With ``slack_peer_groups`` the rule is applied inside each peer group: a rank with data is named iff ITS GROUP waits
        (the group's ``typical_share >= min_share`` and ``typical_waited_us > 0``) and the rank hardly does (``waited_us <=
        max_ratio *`` the group's typical wait).  The typical wait is a lower median: in a group of two it is the late rank's
        own wait, about 0, so a group of two names nobody; a rank alone in its group is unrated."""
        s = self.slack_scores()
        share = s.get("min_share", 0.05) if min_share is None else min_share
        ratio = s.get("max_ratio", 0.25) if max_ratio is None else max_ratio
        for name, v in (("min_share", share), ("max_ratio", ratio)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not v >= 0:
                raise ValueError(f"{name} must be a number >= 0, got {v!r}")
        named = []
        if s.get("peer_groups"):
            for r, rec in s["ranks"].items():
                grp = s["per_group"][rec["group"]]
                if grp["typical_share"] >= share and grp["typical_waited_us"] > 0 and rec["waited_us"] <= ratio * grp["typical_waited_us"]:
                    named.append(r)
        elif s and s["typical_share"] >= share and s["typical_waited_us"] > 0:
            limit = ratio * s["typical_waited_us"]
            named = [r for r, rec in s["ranks"].items() if rec["waited_us"] <= limit]
        return {"straggler_gpus_slack": self._ids(named)}

    def _family_scores(self, name: str) -> Dict[str, Any]:
        """A private copy of one row family's scores (built from the device's planes on first use); ``{}`` without them.

        With ``ReportGenerator(row_peer_groups=True)`` the reference of a column is the smallest value among the rank's OWN peer
        group that has the row, and the dict gains ``"peer_groups": True``, ``"min_peers"``, ``"groups"``, ``"group_of"``,
        ``"unrated_ranks"`` as ``peer_scores()`` spells them, and ``"section_reference"`` / ``"kernel_reference"``: ``{name:
        {group label: {"value": the group's reference, "rank": the lowest rank that holds it, "ranks": how many of the group
        have the row}}}`` of the pairs at least ``min_peers`` ranks have."""
        fam = row_families.BY_NAME[name]
        scores = self.__dict__.get(fam.slot)
        if scores is None:
            return {}
        if isinstance(scores, _RowFamilySource):
            scores = self.__dict__[fam.slot] = scores.build()
        out = _copy_scores(scores)
        for alias, key in fam.aliases:
            out[alias] = out[key]
        if out.get("peer_groups"):  # (row_peer_groups: the lists are private copies too)
            out["groups"] = {label: list(members) for label, members in out["groups"].items()}
            out["unrated_ranks"] = list(out["unrated_ranks"])
        return out

    def _identify_relative(self, scores: Mapping[str, Any], gpu_thr: float, sec_thr: float) -> Dict[str, Any]:
        gr = self._below(scores.get("gpu_relative", {}), gpu_thr)
        sr = {n: self._below(v, sec_thr) for n, v in scores.get("section_relative", {}).items()}
        return {"straggler_gpus_relative": self._ids(gr),
                "straggler_sections_relative": {n: self._ids(r) for n, r in sr.items() if r}}

    def _ids(self, ranks) -> set:
        return {StragglerId(rank=r, node=self.rank_to_node[r]) for r in ranks}

    @staticmethod
    def _below(scores: Mapping[int, float], threshold: float):
        return [r for r, s in scores.items() if s < threshold]

    def identify_stragglers(
        self,
        gpu_rel_threshold: float = 0.75,
        section_rel_threshold: float = 0.75,
        gpu_indiv_threshold: float = 0.75,
        section_indiv_threshold: float = 0.75,
    ) -> Dict[str, Any]:
        """Ranks whose scores fall strictly below the thresholds (NaN scores are never flagged).

        Returns ``{'straggler_gpus_relative': set[StragglerId], 'straggler_gpus_individual': set,
        'straggler_sections_relative': {section: set}, 'straggler_sections_individual': {section:
        set}}``; a section appears only if at least one rank is flagged for it.
        """
        src = self.__dict__.get("_src")
        if src is not None and src.view.layout is not None:
            fast = src.flagged(self.rank_to_node, (gpu_rel_threshold, section_rel_threshold, gpu_indiv_threshold,
                                                   section_indiv_threshold))
            if fast is not None:
                return fast
        flags = self._flags()
        if flags is not None and flags.matches(
            gpu_rel_threshold, section_rel_threshold, gpu_indiv_threshold, section_indiv_threshold
        ):
            # thresholds equal the ones the score kernel was launched with: use its flag bytes
            src = self.__dict__.get("_src")
            ids = src.view.straggler_ids(self.rank_to_node) if src is not None else None
            gr, gi, sr, si = flags.decode(ids, src.view.memo() if src is not None else None)
            if ids is not None:
                return {"straggler_gpus_relative": gr, "straggler_gpus_individual": gi,
                        "straggler_sections_relative": sr, "straggler_sections_individual": si}
        else:
            gr = self._below(self.gpu_relative_perf_scores, gpu_rel_threshold)
            gi = self._below(self.gpu_individual_perf_scores, gpu_indiv_threshold)
            sr = {n: self._below(v, section_rel_threshold) for n, v in self.section_relative_perf_scores.items()}
            si = {n: self._below(v, section_indiv_threshold) for n, v in self.section_individual_perf_scores.items()}
        return {
            "straggler_gpus_relative": self._ids(gr),
            "straggler_gpus_individual": self._ids(gi),
            "straggler_sections_relative": {n: self._ids(r) for n, r in sr.items() if r},
            "straggler_sections_individual": {n: self._ids(r) for n, r in si.items() if r},
        }


class _DeviceFlags:
    """Below-threshold bytes written by the score kernel, with the thresholds they were computed for.
    Holds a private ndarray (never a view of the live result block, never a callable): picklable.  ``flags`` may
    be given as a ``_ScoreSource`` whose block is still in flight; it is resolved on first use."""

    __slots__ = ("thresholds", "flags", "ranks", "names", "cols", "S", "has_rel", "has_indiv")

    def __init__(self, thresholds, flags, ranks, names, cols, S, has_rel, has_indiv):
        self.thresholds = thresholds  # (gpu_rel, sec_rel, gpu_indiv, sec_indiv), a tuple of floats
        self.flags = flags  # ndarray [ranks, 2+2S] u8, or the _ScoreSource that will hold it
        self.ranks = ranks
        self.names = names
        self.cols = cols if isinstance(cols, dict) else dict(zip(names, cols))
        self.S = S
        self.has_rel = has_rel
        self.has_indiv = has_indiv

    def _array(self) -> np.ndarray:
        f = self.flags
        if isinstance(f, _ScoreSource):
            f = self.flags = f.ensure().flags
        return f

    def __getstate__(self):
        self._array()
        return {k: getattr(self, k) for k in self.__slots__}

    def __setstate__(self, state) -> None:
        for k, v in state.items():
            setattr(self, k, v)

    def matches(self, gpu_rel, sec_rel, gpu_indiv, sec_indiv) -> bool:
        return (float(gpu_rel), float(sec_rel), float(gpu_indiv), float(sec_indiv)) == self.thresholds

    def decode(self, ids=None, memo=None):
        """Flagged rows per score family: ``(gpu_rel, gpu_indiv, section_rel, section_indiv)``.  With ``ids`` (one
        ``StragglerId`` per row of the table) the results are the sets ``identify_stragglers`` returns; without, lists
        of ranks.  One ``any()`` in the common case (nothing flagged).  Otherwise per-column counts and first flagged
        rows come from two reductions over the table and only flagged columns are visited.  ``memo`` (a dict shared by
        the reports of one plan): a straggler usually stays one for many reports, so the result for an unchanged flag
        table is kept and handed out as fresh copies (a set copy does not re-hash its members)."""
        S = self.S
        wrap = set if ids is not None else list
        src = self.flags
        fb = src.flag_bytes() if isinstance(src, _ScoreSource) else src.tobytes()
        if fb.count(0) == len(fb):  # (bytes.count: one C loop, no numpy call on the common path)
            return wrap(), wrap(), {}, {}
        key = None
        if memo is not None and ids is not None:
            key = fb
            hit = memo.get("flags")
            if hit is not None and hit[0] == key and hit[1] is ids:
                gr, gi, sr, si = hit[2]
                return gr.copy(), gi.copy(), _copy_sets(sr), _copy_sets(si)
        f = self._array()
        who = ids if ids is not None else self.ranks
        cnt = f.sum(axis=0, dtype=np.int32).tolist()
        first = f.argmax(axis=0).tolist()

        def members(c):
            if cnt[c] == 1:
                return wrap((who[first[c]],))
            return wrap(who[int(r)] for r in np.flatnonzero(f[:, c]))

        gi = members(0) if (self.has_indiv and cnt[0]) else wrap()
        gr = members(1) if (self.has_rel and cnt[1]) else wrap()
        si: Dict[str, Any] = {}
        sr: Dict[str, Any] = {}
        if any(cnt[2:]):
            cols = self.cols
            # the report's own section order, as the reference's walk over its score dicts gives it
            if self.has_indiv:
                si = {n: members(2 + cols[n]) for n in self.names if cnt[2 + cols[n]]}
            if self.has_rel:
                sr = {n: members(2 + S + cols[n]) for n in self.names if cnt[2 + S + cols[n]]}
        if key is not None:
            memo["flags"] = (key, ids, (gr.copy(), gi.copy(), _copy_sets(sr), _copy_sets(si)))
        return gr, gi, sr, si


def steps_behind_report(generator) -> tuple:
    """Whether steps follow a report of ``generator``: ``(any table follow-up, any ring step)``, by its options alone
    (``peer_history``, the trends and the per-peer-group variants need one of these).  The generator asks once, in its
    ``__init__``; ``straggler._Lane.build`` asks for whatever it is handed, so an option that is not there counts as off."""
    table = bool(getattr(generator, "kernel_attribution", 0) or getattr(generator, "robust_scores", False)
                 or getattr(generator, "work_groups", False) or getattr(generator, "peer_groups", None) is not None
                 or getattr(generator, "pace_scores", False) or getattr(generator, "node_scores", False)
                 or getattr(generator, "score_history", 0))
    ring = bool(any(getattr(generator, fam.param_attrs[0], 0) for fam in row_families.FAMILIES)
                or getattr(generator, "collective_slack", False))
    return table, ring


class ReportGenerator:
    """Builds :class:`Report` objects; every rank of the group must call ``generate_report`` together.

    Args:
        scores_to_compute: any of ``'relative_perf_scores'``, ``'individual_perf_scores'``.
        gather_on_rank0: rank 0's report covers all ranks and the other ranks return ``None``;
            otherwise every rank reports only itself.
        pg: process group (default: WORLD).
        node_name: name of this node in ``rank_to_node``.
        thresholds: (gpu_rel, section_rel, gpu_indiv, section_indiv) the score kernel pre-computes
            straggler flags for (default 0.75 each, the ``identify_stragglers`` defaults).
        asynchronous: steady-state ring reports are only ENQUEUED (statistics kernel, collective, score kernel on
            the detector's stream) and the returned ``Report`` waits for them when it is first read, so the training
            loop never stalls on a report.  Not in the reference, whose ``generate_report`` is synchronous; two
            visible differences: ``generate_report_elapsed_time`` is the enqueue time, and a name that first appears
            on some rank enters the reports one report later (the name exchange is a host collective and runs at the
            start of the next ``generate_report``, when every rank is there).
    """

    def __init__(self, scores_to_compute, gather_on_rank0=True, pg=None, node_name="<notset>",
                 thresholds: Sequence[float] = _backend_mod.DEFAULT_THRESHOLDS, asynchronous: bool = False,
                 kernel_attribution: int = 0, tail_quantile: float = 0.0, robust_scores: bool = False,
                 robust_min_ranks: int = 4, robust_floor: float = 0.02, onset_detection: bool = False,
                 onset_min_segment: float = 0.05, onset_min_strength: float = 0.5, period_detection: bool = False,
                 period_max: int = 1024, period_min_strength: float = 0.5, episode_detection: bool = False,
                 episode_min_length: float = 0.005, episode_min_strength: float = 0.5, score_history: int = 0,
                 persistence_min_reports: int = 3, persistence_thresholds: Optional[Sequence[float]] = None,
                 score_trends: bool = False, trend_min_reports: int = 6, trend_min_tau: float = 0.6,
                 trend_horizon: Optional[int] = None, collective_slack: bool = False, slack_min_ranks: int = 4,
                 slack_min_share: float = 0.05, slack_max_ratio: float = 0.25, peer_groups=None,
                 peer_min_ranks: int = 2, peer_history: int = 0, peer_persistence_min_reports: int = 3,
                 peer_persistence_thresholds: Optional[Sequence[float]] = None, peer_trends: bool = False,
                 pace_scores: bool = False, pace_min_ranks: int = 4, pace_min_columns: int = 8,
                 pace_min_effect: float = 0.03, pace_min_breadth: float = 0.9, pace_peer_groups: bool = False,
                 node_scores: bool = False, node_groups=None, node_min_members: int = 2, node_min_nodes: int = 3,
                 node_min_columns: int = 8, node_min_effect: float = 0.03, node_min_breadth: float = 0.9,
                 node_min_agree: float = 0.75, work_groups: bool = False, work_count_tol: float = 0.25,
                 work_max_unlike: float = 0.1, slack_peer_groups: bool = False, row_peer_groups: bool = False) -> None:
        self.is_computing_rel_scores = "relative_perf_scores" in scores_to_compute
        self.is_computing_indiv_scores = "individual_perf_scores" in scores_to_compute
        self.gather_on_rank0 = gather_on_rank0
        self.group = pg
        self.world_size = dist_utils.get_world_size(self.group)
        self.rank = dist_utils.get_rank(self.group)
        self.node_name = node_name
        self.thresholds = tuple(float(t) for t in thresholds)

        # best medians seen on this rank (individual-score reference); host copy used by the
        # dict-input path, the ring path keeps its own copy in HBM next to the rings
        self.min_local_kernel_times: Dict[str, float] = collections.defaultdict(lambda: float("inf"))
        self.min_local_section_times: Dict[str, float] = collections.defaultdict(lambda: float("inf"))

        self.name_mapper = NameMapper(pg=pg)
        # ids for the "nothing is exchanged" mode (individual scores, no gather): stays local so
        # that ``name_mapper`` is untouched, as the reference guarantees
        self._private_mapper = NameMapper(pg=pg)
        self.rank_to_node: Dict[int, str] = collections.defaultdict(lambda: "<unk>")
        self._rank_to_node_folded = False  # rank_to_node already names every LOGICAL rank of a folded job (local_ranks > 1)
        # the per-report all-gather straight into RCCL on our own stream (rccl_direct.py); created
        # collectively on the first multi-rank report, None = stay on torch.distributed
        self._direct = None
        self._direct_tried = False
        # asynchronous reports (ring path only): generate_report_from_rings enqueues the report and returns a Report
        # that waits for the device on first read; the block in flight is settled before the next report starts
        self.asynchronous = bool(asynchronous)
        self.exchange_info: Dict[str, Any] = {}
        # ---- when ranks sync names and which collectives a ring report issues (transition table: DESIGN.md section 4).  Written
        # by this class alone; Detector's lane reads them, and mirrors two writes on its hot path (straggler._Lane.run) ----
        self._ring_plan = None        # the cached steady-state plan (_RingPlan); None: the next ring report takes the general path
        self._ring_gid_state = None   # (mapper, version, rows, workspace) the GENERAL path last pointed the ring rows at; None: stale
        self._inflight: Optional[_PendingBlock] = None  # the asynchronous report that was enqueued and nobody has seen complete
        self._prev_async_settled = True  # no asynchronous report of this generator is unaccounted for (see _settle_inflight)
        self._resync_pending = False  # some rank's table said "ids missing": no plan, no lane; the general path syncs names first
        self._had_ring_report = False  # a ring report has reached its score round (collective: the same on every rank)
        self._unreported_rows: list = []  # see take_unreported_rows
        # a synchronous one-call report is issued, its Report built (and the rings emptied, when the caller asked) while the
        # GPU runs, and only then waited for -- where the rings can (report_issue / report_wait) and no exchange runs inside
        # the call; NVRX_DEBUG_REPORT_SPLIT=0 (read here, once) keeps the one call
        self._report_split = os.environ.get("NVRX_DEBUG_REPORT_SPLIT", "1") != "0"
        self._rings_were_reset = False  # the planned report that just ran emptied the rings itself (reset_rings)
        # kernel attribution: every report also names the top-N kernels behind each GPU score (Report.explain_gpu_scores); 0 = off:
        # no buffer, no launch, no backend call.  Every rank should pass the same value (it changes no collective, so a
        # mismatch cannot hang anything: a rank's own reports simply carry what that rank asked for)
        n = int(kernel_attribution)
        if not 0 <= n <= 16:
            raise ValueError(f"kernel_attribution must be 0 (off) or 1..16 kernels per GPU score, got {kernel_attribution!r}")
        self.kernel_attribution = n
        if n:
            be = _backend_mod._backend  # (an engine that does not exist yet is the HIP engine, which has it)
            if be is not None and not hasattr(be, "attribute"):
                raise RuntimeError(f"kernel_attribution={n}: the active backend ({getattr(be, 'name', type(be).__name__)}) "
                                   "has no kernel attribution (backend.attribute)")
        self._attr_names_cache = (None, 0, ())  # (mapper, kernel ids covered, names by id)
        # tail scores: every ring report also carries the q-quantile of every row and relative scores built from them
        # (Report.tail_scores); 0 = off: no buffer, no launch, no collective, no backend call.  The step adds one collective
        # per report, so EVERY rank must pass the same value.
        self.tail_q_ppm = _backend_mod._native.tail_q_ppm(tail_quantile)
        if self.tail_q_ppm:
            if not self.is_computing_rel_scores:
                raise ValueError(f"tail_quantile={tail_quantile!r} needs relative_perf_scores among scores_to_compute "
                                 f"(got {scores_to_compute!r}): tail scores are relative scores")
            be = _backend_mod._backend  # (an engine that does not exist yet is the HIP engine, which has it)
            if be is not None and not hasattr(be, "tail_score"):
                raise RuntimeError(f"tail_quantile={tail_quantile!r}: the active backend ({getattr(be, 'name', type(be).__name__)}) "
                                   "has no tail scores (backend.tail_score)")
        # robust scores: every report also rates each rank against the job's median and spread (Report.robust_scores); off: no
        # buffer, no launch, no backend call.  They read the exchanged table only: no collective, so a mismatch between ranks
        # cannot hang anything -- but every rank should pass the same value.
        self.robust_scores = bool(robust_scores)
        if self.robust_scores:
            if isinstance(robust_min_ranks, bool) or not isinstance(robust_min_ranks, (int, np.integer)) or robust_min_ranks < 1:
                raise ValueError(f"robust_min_ranks must be an integer >= 1, got {robust_min_ranks!r}")
            try:
                floor = float(robust_floor)
            except (TypeError, ValueError):
                raise ValueError(f"robust_floor must be a number within [0, 1], got {robust_floor!r}") from None
            if not 0.0 <= floor <= 1.0:  # (NaN fails both comparisons)
                raise ValueError(f"robust_floor must be within [0, 1], got {robust_floor!r}")
            if not self.is_computing_rel_scores:
                raise ValueError(f"robust_scores needs relative_perf_scores among scores_to_compute (got {scores_to_compute!r}): "
                                 "robust scores are relative scores")
            be = _backend_mod._backend  # (an engine that does not exist yet is the HIP engine, which has it)
            if be is not None and not hasattr(be, "robust_score"):
                raise RuntimeError(f"robust_scores: the active backend ({getattr(be, 'name', type(be).__name__)}) "
                                   "has no robust scores (backend.robust_score)")
            self.robust_min_ranks, self.robust_floor = int(robust_min_ranks), floor
        # peer-group scores: every report also rates each rank against the fastest rank of its own group -- the ranks doing the
        # same work (Report.peer_scores); None = off: no buffer, no launch, no backend call.  They read the exchanged table
        # only: no collective, so a mismatch between ranks cannot hang anything -- but every rank should pass the same value.
        self.peer_groups = _peer_spec(peer_groups)  # None, a backend._PeerRule or a tuple of labels, one per logical rank
        self._peer_resolved = None  # backend.PeerGroups for the R of the tables seen so far
        if self.peer_groups is not None:
            if isinstance(peer_min_ranks, bool) or not isinstance(peer_min_ranks, (int, np.integer)) or peer_min_ranks < 1:
                raise ValueError(f"peer_min_ranks must be an integer >= 1, got {peer_min_ranks!r}")
            if not self.is_computing_rel_scores:
                raise ValueError(f"peer_groups needs relative_perf_scores among scores_to_compute (got {scores_to_compute!r}): "
                                 "peer-group scores are relative scores")
            be = _backend_mod._backend  # (an engine that does not exist yet is the HIP engine, which has it)
            if be is not None and not hasattr(be, "peer_score"):
                raise RuntimeError(f"peer_groups: the active backend ({getattr(be, 'name', type(be).__name__)}) "
                                   "has no peer-group scores (backend.peer_score)")
            self.peer_min_ranks = int(peer_min_ranks)
        # work groups: every report also says which ranks do the same work, inferred from the table (Report.work_groups), and
        # peer_groups="auto" takes its groups from there; off: no buffer, no launch, no backend call.  The step reads the
        # exchanged table only: no collective, and every rank infers the same groups from the same table.  0.25 and 0.1 are
        # defaults, not measurements.
        self.work_groups = bool(work_groups) or self.peer_groups == "auto"
        self._work_handle = None  # this report's step (peer_groups="auto" waits for it: _peer_for)
        self._peer_auto_roots = None  # the root array _peer_resolved was built from
        if self.work_groups:
            try:
                tol, share = float(work_count_tol), float(work_max_unlike)
            except (TypeError, ValueError):
                raise ValueError(f"work_count_tol and work_max_unlike must be numbers, got {work_count_tol!r} and "
                                 f"{work_max_unlike!r}") from None
            if isinstance(work_count_tol, bool) or not 0.0 <= tol <= 16.0:  # (NaN fails both comparisons)
                raise ValueError(f"work_count_tol must be within [0, 16], got {work_count_tol!r}")
            if isinstance(work_max_unlike, bool) or not 0.0 <= share <= 1.0:
                raise ValueError(f"work_max_unlike must be within [0, 1], got {work_max_unlike!r}")
            option = "peer_groups='auto'" if self.peer_groups == "auto" else "work_groups"
            if not self.is_computing_rel_scores:
                raise ValueError(f"{option} needs relative_perf_scores among scores_to_compute (got {scores_to_compute!r}): "
                                 "work groups compare ranks")
            be = _backend_mod._backend  # (an engine that does not exist yet is the HIP engine, which has it)
            if be is not None and not hasattr(be, "work_groups"):
                raise RuntimeError(f"{option}: the active backend ({getattr(be, 'name', type(be).__name__)}) "
                                   "has no work groups (backend.work_groups)")
            self.work_count_tol, self.work_max_unlike = tol, share
            self.work_max_unlike_ppm = int(round(share * 1e6))
        # pace scores: every report also says whether a rank is a little slower in nearly all of its kernels
        # (Report.pace_scores); off: no buffer, no launch, no backend call.  They read the exchanged table only: no collective,
        # so a mismatch between ranks cannot hang anything -- but every rank should pass the same value.
        self.pace_scores = bool(pace_scores)
        if self.pace_scores:
            if isinstance(pace_min_ranks, bool) or not isinstance(pace_min_ranks, (int, np.integer)) or pace_min_ranks < 1:
                raise ValueError(f"pace_min_ranks must be an integer >= 1, got {pace_min_ranks!r}")
            if isinstance(pace_min_columns, bool) or not isinstance(pace_min_columns, (int, np.integer)) or pace_min_columns < 1:
                raise ValueError(f"pace_min_columns must be an integer >= 1, got {pace_min_columns!r}")
            try:
                effect, breadth = float(pace_min_effect), float(pace_min_breadth)
            except (TypeError, ValueError):
                raise ValueError(f"pace_min_effect and pace_min_breadth must be numbers, got {pace_min_effect!r} and "
                                 f"{pace_min_breadth!r}") from None
            if not 0.0 <= effect < 1.0:
                raise ValueError(f"pace_min_effect must be within [0, 1), got {pace_min_effect!r}")
            if not 0.0 < breadth <= 1.0:
                raise ValueError(f"pace_min_breadth must be within (0, 1], got {pace_min_breadth!r}")
            if not self.is_computing_rel_scores:
                raise ValueError(f"pace_scores needs relative_perf_scores among scores_to_compute (got {scores_to_compute!r}): "
                                 "pace scores are relative scores")
            be = _backend_mod._backend  # (an engine that does not exist yet is the HIP engine, which has it)
            if be is not None and not hasattr(be, "pace_score"):
                raise RuntimeError(f"pace_scores: the active backend ({getattr(be, 'name', type(be).__name__)}) "
                                   "has no pace scores (backend.pace_score)")
            self.pace_min_ranks, self.pace_min_columns = int(pace_min_ranks), int(pace_min_columns)
            self.pace_min_effect, self.pace_min_breadth = effect, breadth
        # pace scores per peer group: the pace step rates each rank against the lower median of its OWN group
        # (nvrx_pace_group_score); off: the pace step is the job-wide one, whatever peer_groups says
        self.pace_peer_groups = bool(pace_peer_groups)
        if self.pace_peer_groups:
            if not self.pace_scores or self.peer_groups is None:
                missing = [name for name, on in (("pace_scores", self.pace_scores), ("peer_groups", self.peer_groups is not None))
                           if not on]
                raise ValueError(f"pace_peer_groups needs pace_scores and peer_groups; {' and '.join(missing)} "
                                 f"{'is' if len(missing) == 1 else 'are'} not set")
            be = _backend_mod._backend  # (an engine that does not exist yet is the HIP engine, which has it)
            if be is not None and not hasattr(be, "pace_group_score"):
                raise RuntimeError(f"pace_peer_groups: the active backend ({getattr(be, 'name', type(be).__name__)}) "
                                   "has no pace scores per peer group (backend.pace_group_score)")
        # node scores: every report also says whether a NODE is a little slower in nearly all of its kernels (Report.node_scores);
        # off: nothing is allocated, resolved, launched or called.  They read the exchanged table and rank_to_node only: no
        # collective, so ranks need not agree on the option.
        self.node_scores = bool(node_scores)
        self.node_groups = None
        self._node_resolved = None  # backend.PeerGroups of the nodes for the R (and rank_to_node) of the tables seen so far
        self._node_source = None    # the rank_to_node object _node_resolved was built from (node_groups=None)
        if self.node_scores:
            for name, val in (("node_min_members", node_min_members), ("node_min_nodes", node_min_nodes),
                              ("node_min_columns", node_min_columns)):
                if isinstance(val, bool) or not isinstance(val, (int, np.integer)) or val < 1:
                    raise ValueError(f"{name} must be an integer >= 1, got {val!r}")
            try:
                effect, breadth, agree = float(node_min_effect), float(node_min_breadth), float(node_min_agree)
            except (TypeError, ValueError):
                raise ValueError(f"node_min_effect, node_min_breadth and node_min_agree must be numbers, got {node_min_effect!r}, "
                                 f"{node_min_breadth!r} and {node_min_agree!r}") from None
            if not 0.0 <= effect < 1.0:
                raise ValueError(f"node_min_effect must be within [0, 1), got {node_min_effect!r}")
            if not 0.0 < breadth <= 1.0:
                raise ValueError(f"node_min_breadth must be within (0, 1], got {node_min_breadth!r}")
            if not 0.0 < agree <= 1.0:
                raise ValueError(f"node_min_agree must be within (0, 1], got {node_min_agree!r}")
            if not self.is_computing_rel_scores:
                raise ValueError(f"node_scores needs relative_perf_scores among scores_to_compute (got {scores_to_compute!r}): "
                                 "node scores are relative scores")
            be = _backend_mod._backend  # (an engine that does not exist yet is the HIP engine, which has it)
            if be is not None and not hasattr(be, "node_score"):
                raise RuntimeError(f"node_scores: the active backend ({getattr(be, 'name', type(be).__name__)}) "
                                   "has no node scores (backend.node_score)")
            self.node_groups = _peer_spec(node_groups, "node_groups")  # None: the nodes are rank_to_node's
            self.node_min_members, self.node_min_nodes = int(node_min_members), int(node_min_nodes)
            self.node_min_columns = int(node_min_columns)
            self.node_min_effect, self.node_min_breadth, self.node_min_agree = effect, breadth, agree
        # onset scores: every ring report also carries, per row, the single step that explains most of the window's variance and
        # relative scores built from the shifts (Report.onset_scores); off: no buffer, no launch, no collective, no backend
        # call.  The step adds one collective per report, so EVERY rank must pass the same value.
        self.onset_seg_ppm = 0  # (0 = off)
        if onset_detection:
            seg_ppm = _backend_mod._native.onset_seg_ppm(onset_min_segment)
            try:
                strength = float(onset_min_strength)
            except (TypeError, ValueError):
                raise ValueError(f"onset_min_strength must be a number within [0, 1], got {onset_min_strength!r}") from None
            if not 0.0 <= strength <= 1.0:  # (NaN fails both comparisons)
                raise ValueError(f"onset_min_strength must be within [0, 1], got {onset_min_strength!r}")
            if not self.is_computing_rel_scores:
                raise ValueError(f"onset_detection needs relative_perf_scores among scores_to_compute (got {scores_to_compute!r}): "
                                 "onset scores are relative scores")
            be = _backend_mod._backend  # (an engine that does not exist yet is the HIP engine, which has it)
            if be is not None and not hasattr(be, "onset_score"):
                raise RuntimeError(f"onset_detection: the active backend ({getattr(be, 'name', type(be).__name__)}) "
                                   "has no onset scores (backend.onset_score)")
            self.onset_seg_ppm, self.onset_min_strength = seg_ppm, strength
        # period scores: every ring report also carries, per row, the period on which the row stalls, if any, and relative
        # scores built from the excesses (Report.period_scores); off: no buffer, no launch, no collective, no backend call.
        # The step adds one collective per report, so EVERY rank must pass the same value.
        self.period_max = 0  # (0 = off)
        if period_detection:
            pmax = _backend_mod._native.period_max(period_max)
            try:
                strength = float(period_min_strength)
            except (TypeError, ValueError):
                raise ValueError(f"period_min_strength must be a number within [0, 1], got {period_min_strength!r}") from None
            if not 0.0 <= strength <= 1.0:  # (NaN fails both comparisons)
                raise ValueError(f"period_min_strength must be within [0, 1], got {period_min_strength!r}")
            if not self.is_computing_rel_scores:
                raise ValueError(f"period_detection needs relative_perf_scores among scores_to_compute (got {scores_to_compute!r}): "
                                 "period scores are relative scores")
            be = _backend_mod._backend  # (an engine that does not exist yet is the HIP engine, which has it)
            if be is not None and not hasattr(be, "period_score"):
                raise RuntimeError(f"period_detection: the active backend ({getattr(be, 'name', type(be).__name__)}) "
                                   "has no period scores (backend.period_score)")
            self.period_max, self.period_min_strength = pmax, strength
        # episode scores: every ring report also carries, per row, the one stretch of the window that spent most time above
        # the row's mean, if any, and relative scores built from the excesses (Report.episode_scores); off: no buffer, no
        # launch, no collective, no backend call.  The step adds one collective per report, so EVERY rank must pass the same
        # value.
        self.episode_len_ppm = 0  # (0 = off)
        if episode_detection:
            len_ppm = _backend_mod._native.episode_len_ppm(episode_min_length)
            try:
                strength = float(episode_min_strength)
            except (TypeError, ValueError):
                raise ValueError(f"episode_min_strength must be a number within [0, 1], got {episode_min_strength!r}") from None
            if not 0.0 <= strength <= 1.0:  # (NaN fails both comparisons)
                raise ValueError(f"episode_min_strength must be within [0, 1], got {episode_min_strength!r}")
            if not self.is_computing_rel_scores:
                raise ValueError(f"episode_detection needs relative_perf_scores among scores_to_compute (got {scores_to_compute!r}): "
                                 "episode scores are relative scores")
            be = _backend_mod._backend  # (an engine that does not exist yet is the HIP engine, which has it)
            if be is not None and not hasattr(be, "episode_score"):
                raise RuntimeError(f"episode_detection: the active backend ({getattr(be, 'name', type(be).__name__)}) "
                                   "has no episode scores (backend.episode_score)")
            self.episode_len_ppm, self.episode_min_strength = len_ppm, strength
        # score history: every report also appends its scores to a device ring of the last H reports and says, per rank and
        # score, for how many reports in a row the score has been below its threshold (Report.score_history,
        # Report.identify_persistent_stragglers); 0 = off: no buffer, no launch, no backend call.  It reads what the score
        # kernel wrote: no collective, so a mismatch between ranks cannot hang anything.  The history belongs to this generator
        # and dies with it.
        self._history = None  # (backend.ScoreHistory while the option is on)
        depth = score_history
        if isinstance(depth, bool) or not isinstance(depth, (int, np.integer)) or not (
                depth == 0 or 2 <= depth <= _backend_mod._native.HISTORY_MAX_DEPTH):
            raise ValueError(f"score_history must be 0 (off) or an integer within [2, {_backend_mod._native.HISTORY_MAX_DEPTH}] "
                             f"reports, got {score_history!r}")
        self.score_history = int(depth)
        if self.score_history:
            m = persistence_min_reports
            if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or not 1 <= m <= self.score_history:
                raise ValueError(f"persistence_min_reports must be an integer within [1, score_history={self.score_history}], "
                                 f"got {persistence_min_reports!r}")
            try:
                thr = self.thresholds if persistence_thresholds is None else tuple(float(t) for t in persistence_thresholds)
            except (TypeError, ValueError):
                raise ValueError(f"persistence_thresholds must be four finite numbers (gpu_rel, section_rel, gpu_indiv, "
                                 f"section_indiv), got {persistence_thresholds!r}") from None
            if len(thr) != 4 or not all(np.isfinite(thr)):
                raise ValueError(f"persistence_thresholds must be four finite numbers (gpu_rel, section_rel, gpu_indiv, "
                                 f"section_indiv), got {persistence_thresholds!r}")
            be = _backend_mod._backend  # (an engine that does not exist yet is the HIP engine, which has it)
            if be is not None and not hasattr(be, "score_history"):
                raise RuntimeError(f"score_history: the active backend ({getattr(be, 'name', type(be).__name__)}) "
                                   "has no score history (backend.score_history)")
            self.persistence_min_reports, self.persistence_thresholds = int(m), thr
            self._history = _backend_mod.ScoreHistory(self.score_history)
        # score trends: behind the history step, every report also estimates per rank and score whether the ring's scores are
        # falling (Report.score_trends, Report.identify_declining_stragglers); off: no buffer, no launch, no backend call.  It
        # reads the history ring only: no collective.  min_reports 6, min_tau 0.6 and the horizon H are defaults, not
        # measurements.
        self.score_trends = bool(score_trends)
        if self.score_trends:
            if self.score_history < 4:
                raise ValueError(f"score_trends needs a score history of at least 4 reports (score_history within [4, "
                                 f"{_backend_mod._native.HISTORY_MAX_DEPTH}]), got score_history={self.score_history!r}")
            m = trend_min_reports
            if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or not 4 <= m <= self.score_history:
                raise ValueError(f"trend_min_reports must be an integer within [4, score_history={self.score_history}], "
                                 f"got {trend_min_reports!r}")
            try:
                tau = float(trend_min_tau)
            except (TypeError, ValueError):
                tau = float("nan")
            if isinstance(trend_min_tau, bool) or not 0.0 < tau <= 1.0:
                raise ValueError(f"trend_min_tau must be a number within (0, 1], got {trend_min_tau!r}")
            hz = self.score_history if trend_horizon is None else trend_horizon
            if isinstance(hz, bool) or not isinstance(hz, (int, np.integer)) or hz < 0:
                raise ValueError(f"trend_horizon must be None (the history's depth) or an integer >= 0 reports, "
                                 f"got {trend_horizon!r}")
            be = _backend_mod._backend  # (an engine that does not exist yet is the HIP engine, which has it)
            if be is not None and not hasattr(be, "score_trend"):
                raise RuntimeError(f"score_trends: the active backend ({getattr(be, 'name', type(be).__name__)}) "
                                   "has no score trends (backend.score_trend)")
            self.trend_min_reports, self.trend_min_tau, self.trend_horizon = int(m), tau, int(hz)
        # peer-score history and trends: the two options above on the PEER scores (Report.peer_history,
        # Report.identify_persistent_peer_stragglers, Report.peer_trends, Report.identify_declining_peer_stragglers); 0 = off:
        # no buffer, no launch, no backend call.  The step runs directly behind the peer step and reads its rank part where
        # that step wrote it: no collective.  The history is per rank: it does not notice that a rank's peers changed.
        self._peer_history = None  # (backend.PeerHistory while the option is on)
        depth = peer_history
        if isinstance(depth, bool) or not isinstance(depth, (int, np.integer)) or not (
                depth == 0 or 2 <= depth <= _backend_mod._native.HISTORY_MAX_DEPTH):
            raise ValueError(f"peer_history must be 0 (off) or an integer within [2, {_backend_mod._native.HISTORY_MAX_DEPTH}] "
                             f"reports, got {peer_history!r}")
        self.peer_history = int(depth)
        if self.peer_history:
            if self.peer_groups is None:
                raise ValueError("peer_history needs peer_groups: it is the history of the peer-group scores")
            m = peer_persistence_min_reports
            if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or not 1 <= m <= self.peer_history:
                raise ValueError(f"peer_persistence_min_reports must be an integer within [1, peer_history={self.peer_history}], "
                                 f"got {peer_persistence_min_reports!r}")
            try:
                thr = (0.75, 0.75) if peer_persistence_thresholds is None else tuple(float(t) for t in peer_persistence_thresholds)
            except (TypeError, ValueError):
                thr = ()
            if len(thr) != 2 or not all(np.isfinite(thr)):
                raise ValueError(f"peer_persistence_thresholds must be two finite numbers (gpu, section), "
                                 f"got {peer_persistence_thresholds!r}")
            be = _backend_mod._backend  # (an engine that does not exist yet is the HIP engine, which has it)
            if be is not None and not hasattr(be, "peer_history"):
                raise RuntimeError(f"peer_history: the active backend ({getattr(be, 'name', type(be).__name__)}) "
                                   "has no peer-score history (backend.peer_history)")
            self.peer_persistence_min_reports, self.peer_persistence_thresholds = int(m), thr
            self._peer_history = _backend_mod.PeerHistory(self.peer_history)
        self.peer_trends = bool(peer_trends)
        if self.peer_trends:
            if self.peer_history < 4:
                raise ValueError(f"peer_trends needs a peer history of at least 4 reports (peer_history within [4, "
                                 f"{_backend_mod._native.HISTORY_MAX_DEPTH}]), got peer_history={self.peer_history!r}")
            m = trend_min_reports
            if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or not 4 <= m <= self.peer_history:
                raise ValueError(f"trend_min_reports must be an integer within [4, peer_history={self.peer_history}], "
                                 f"got {trend_min_reports!r}")
            try:
                tau = float(trend_min_tau)
            except (TypeError, ValueError):
                tau = float("nan")
            if isinstance(trend_min_tau, bool) or not 0.0 < tau <= 1.0:
                raise ValueError(f"trend_min_tau must be a number within (0, 1], got {trend_min_tau!r}")
            hz = self.peer_history if trend_horizon is None else trend_horizon
            if isinstance(hz, bool) or not isinstance(hz, (int, np.integer)) or hz < 0:
                raise ValueError(f"trend_horizon must be None (the history's depth) or an integer >= 0 reports, "
                                 f"got {trend_horizon!r}")
            be = _backend_mod._backend  # (an engine that does not exist yet is the HIP engine, which has it)
            if be is not None and not hasattr(be, "peer_trend"):
                raise RuntimeError(f"peer_trends: the active backend ({getattr(be, 'name', type(be).__name__)}) "
                                   "has no peer-score trends (backend.peer_trend)")
            self.trend_min_reports, self.trend_min_tau, self.peer_trend_horizon = int(m), tau, int(hz)
        # slack scores: every ring report also says whom the job waits for in collectives (Report.slack_scores,
        # Report.identify_slack_stragglers) from the statistics of the collective kernels' rows, which every other score drops;
        # off: no buffer, no launch, no collective, no backend call.  The step adds one collective per report, so EVERY rank
        # must pass the same value.  4 ranks, 0.05 and 0.25 are defaults, not measurements.
        self.collective_slack = bool(collective_slack)
        if self.collective_slack:
            if isinstance(slack_min_ranks, bool) or not isinstance(slack_min_ranks, (int, np.integer)) or slack_min_ranks < 1:
                raise ValueError(f"slack_min_ranks must be an integer >= 1, got {slack_min_ranks!r}")
            rule = []
            for name, v in (("slack_min_share", slack_min_share), ("slack_max_ratio", slack_max_ratio)):
                try:
                    x = float(v)
                except (TypeError, ValueError):
                    x = float("nan")
                if isinstance(v, bool) or not (x >= 0.0 and math.isfinite(x)):
                    raise ValueError(f"{name} must be a finite number >= 0, got {v!r}")
                rule.append(x)
            if not self.is_computing_rel_scores:
                raise ValueError(f"collective_slack needs relative_perf_scores among scores_to_compute (got "
                                 f"{scores_to_compute!r}): slack scores compare ranks")
            be = _backend_mod._backend  # (an engine that does not exist yet is the HIP engine, which has it)
            if be is not None and not hasattr(be, "slack_score"):
                raise RuntimeError(f"collective_slack: the active backend ({getattr(be, 'name', type(be).__name__)}) "
                                   "has no slack scores (backend.slack_score)")
            self.slack_min_ranks, (self.slack_min_share, self.slack_max_ratio) = int(slack_min_ranks), rule
        # slack scores per peer group: the score step of the slack scores takes a column's floor and the typical wait inside
        # the rank's OWN group (nvrx_slack_group_score); off: the step is the job-wide one, whatever peer_groups says.  The
        # local step and its collective are the same either way.
        self.slack_peer_groups = bool(slack_peer_groups)
        if self.slack_peer_groups:
            if not self.collective_slack or self.peer_groups is None:
                missing = [name for name, on in (("collective_slack", self.collective_slack),
                                                 ("peer_groups", self.peer_groups is not None)) if not on]
                raise ValueError(f"slack_peer_groups needs collective_slack and peer_groups; {' and '.join(missing)} "
                                 f"{'is' if len(missing) == 1 else 'are'} not set")
            be = _backend_mod._backend  # (an engine that does not exist yet is the HIP engine, which has it)
            if be is not None and not hasattr(be, "slack_group_score"):
                raise RuntimeError(f"slack_peer_groups: the active backend ({getattr(be, 'name', type(be).__name__)}) "
                                   "has no slack scores per peer group (backend.slack_group_score)")
        # the row families that are switched on, in the order their steps (and collectives) run in; and the first of them, if
        # any, that needs the ring-start snapshot
        self._row_families = tuple(f for f in row_families.FAMILIES if f.params(self))
        self._starts_family = next((f for f in self._row_families if f.needs_starts), None)
        # row families per peer group: the score step of every row family that is on takes a column's reference inside the
        # rank's OWN group (nvrx_rowfam_group_score); off: the step is the job-wide one, whatever peer_groups says.  The ring
        # kernels, the send rows and the collectives are the same either way.
        self.row_peer_groups = bool(row_peer_groups)
        if self.row_peer_groups:
            if not self._row_families or self.peer_groups is None:
                missing = [name for name, on in (("a row family (" + ", ".join(f.option for f in row_families.FAMILIES) + ")",
                                                  bool(self._row_families)),
                                                 ("peer_groups", self.peer_groups is not None)) if not on]
                raise ValueError(f"row_peer_groups needs a row family and peer_groups; {' and '.join(missing)} "
                                 f"{'is' if len(missing) == 1 else 'are'} not set")
            be = _backend_mod._backend  # (an engine that does not exist yet is the HIP engine, which has it)
            lacks = [f.name + "_group_score" for f in self._row_families if be is not None and not hasattr(be, f.name + "_group_score")]
            if lacks:
                raise RuntimeError(f"row_peer_groups: the active backend ({getattr(be, 'name', type(be).__name__)}) "
                                   f"has no row-family scores per peer group (backend.{lacks[0]})")
        # what follows a report, decided here once (nothing assigns the options later): whether any table follow-up
        # (_follow_ups) is on, whether any ring step (_ring_steps) is, and what the one-call route needs of its rings
        self._table_steps_on, self._ring_steps_on = steps_behind_report(self)
        pace = ("pace_peer_groups", "report_pace_group") if self.pace_peer_groups else ("pace_scores", "report_pace")
        self._one_call_needs = tuple((option, method) for on, option, method in (
            (self.kernel_attribution, f"kernel_attribution={self.kernel_attribution}", "report_attribute"),
            (self.robust_scores, "robust_scores", "report_robust"),
            (self.work_groups, "work_groups", "report_work"), (self.peer_groups is not None, "peer_groups", "report_peer"),
            (self.pace_scores,) + pace, (self.node_scores, "node_scores", "report_node"),
            (self.peer_history, "peer_history", "report_peer_history"), (self.peer_trends, "peer_trends", "report_peer_trend"),
            (self.score_history, "score_history", "report_history"), (self.score_trends, "score_trends", "report_trend")) if on)
        self._last_plan_fused = False
        self._wr_cache: list = [None]  # this generator's remembered (default group, group, (world, rank)): dist_utils.world_and_rank

    # ---- pieces kept from the reference's host logic ----------------------------------------------
    @staticmethod
    def _filter_out_nccl_kernels(kernel_summaries):
        # collective kernels wait for peers, so their duration says nothing about this GPU
        return {k: v for k, v in kernel_summaries.items() if not is_collective_kernel(k)}

    def _shared_rank_to_node(self) -> Dict[int, str]:
        """The mapping handed to reports: the generator's own plain dict (see ``_maybe_gather_rank_to_node``); a generator
        whose mapping is still the initial defaultdict (nothing gathered yet) gets it converted once."""
        r2n = self.rank_to_node
        if type(r2n) is not dict:
            r2n = self.rank_to_node = dict(r2n)
        return r2n

    def _maybe_gather_rank_to_node(self) -> None:
        if self.rank_to_node:
            return
        # a PLAIN dict from here on, replaced (never edited) when it changes: every report of this generator is handed this
        # very object, and the per-plan caches of the straggler ids / flag decoder are keyed on its identity
        if self.gather_on_rank0:
            pairs = dist_utils.all_gather_object((self.rank, self.node_name), self.group)
            self.rank_to_node = dict(pairs)
        else:
            self.rank_to_node = {self.rank: self.node_name}

    def _update_local_min_times(self, kernel_summaries, section_summaries) -> None:
        for name, summ in kernel_summaries.items():
            if summ[Statistic.MED] < self.min_local_kernel_times[name]:
                self.min_local_kernel_times[name] = summ[Statistic.MED]
        for name, summ in section_summaries.items():
            if summ[Statistic.MED] < self.min_local_section_times[name]:
                self.min_local_section_times[name] = summ[Statistic.MED]

    # ---- kernel attribution ------------------------------------------------------------------------
    def _attr_names(self, mapper, K: int) -> tuple:
        """Kernel names by id, as ``mapper`` has them now (ids are only ever appended: cached until K grows)."""
        owner, n, names = self._attr_names_cache
        if owner is not mapper or n != K:
            names = tuple(mapper.id_to_kernel_name[i] for i in range(K))
            self._attr_names_cache = (mapper, K, names)
        return names

    def _attr_source(self, handle, ws, mapper, lo: int, hi: int, ranks) -> _AttrSource:
        assert handle.first_rank == lo and handle.n_ranks == hi - lo
        return _AttrSource(handle, ranks, self._attr_names(mapper, ws.K), self.is_computing_rel_scores,
                           self.is_computing_indiv_scores)

    # ---- the shared score round -------------------------------------------------------------------
    def _exchanged(self) -> bool:
        return self.is_computing_rel_scores or self.gather_on_rank0

    def _maybe_create_direct_exchange(self) -> None:
        """Collective, once: every rank calls this at the top of its first exchanging report.  Builds the in-stream
        exchange routes -- ``ncclAllGather`` on a communicator of our own (rccl_direct) and, inside one node, direct
        xGMI peer stores into IPC-mapped windows (peer_exchange) -- and keeps the one ``peer_exchange.choose`` picks."""
        if self._direct_tried or self.world_size == 1 or not self._exchanged():
            return
        self._direct_tried = True
        be = _backend_mod.get_backend()
        from . import peer_exchange, rccl_direct

        mode = peer_exchange.exchange_mode()
        if self._ring_steps_on:
            # a row family's collective -- and the slack step's -- is a torch.distributed call between two kernels: reports
            # with one stay on that route as a whole (the option has the same value on every rank, so every rank decides alike
            # -- no collective here).  A row family that is on is the one named.
            option, what = ((self._row_families[0].option, self._row_families[0].name) if self._row_families
                            else ("collective_slack", "slack"))
            self._direct = None
            self.exchange_info = {"route": f"torch.distributed all-gather on the job's own process group ({option} is "
                                           f"set: reports with {what} scores do not use the in-stream routes)", "mode": "c10d"}
            if mode != "c10d":
                _LOG.warning("nvrx straggler: NVRX_EXCHANGE=%s is ignored while %s is set: reports with %s scores "
                             "run on torch.distributed's route (c10d)", mode, option, what)
            return
        # c10d (the default) on ANY rank keeps every rank on torch.distributed (the decision has to be the same everywhere:
        # building a communicator is collective)
        if not dist_utils.is_all_true(mode != "c10d", self.group):
            self._direct = None
            self.exchange_info = {"route": "torch.distributed all-gather on the job's own process group (NVRX_EXCHANGE=c10d, the "
                                           "default; rccl | peer | auto select an in-stream route)", "mode": "c10d"}
            if self.rank == 0:
                _LOG.info("straggler report exchange route: %s", self.exchange_info["route"])
                if self.asynchronous:
                    # torch.distributed's collective is issued by the host, between the statistics and the score kernel: a
                    # report on this route is complete when generate_report returns, whatever `asynchronous` says
                    _LOG.warning("nvrx straggler: asynchronous=True has no effect on the default exchange route (c10d: the report's "
                                 "all-gather is a torch.distributed call on the job's process group, and generate_report() waits for "
                                 "the scores); NVRX_EXCHANGE=rccl | peer | auto selects an in-stream route whose reports are only enqueued")
            return
        maker = getattr(be, "create_direct_exchange", None)  # a test backend may bring its own in-call exchange
        if maker is not None:
            self._direct = maker(self.group)
            return
        index = getattr(be.device, "index", None)
        # the exchange kernel gives up a little BEFORE the host's wait for the completion word does: a peer that is
        # later than the report timeout then surfaces as the exchange's own error (NaN rows, error word, the next
        # report unaffected) instead of a timed-out wait that retires the workspace under a still-spinning kernel
        peer_wait_s = 0.9 * _backend_mod.report_timeout_s() or 1e9
        rccl = rccl_direct.create(self.group, index)
        peer = None
        if mode != "rccl" and (rccl is not None or mode == "peer"):
            # windows need a group that can reach every rank's GPU: built next to the RCCL route (a gloo group whose
            # ranks share one GPU qualifies too when asked for explicitly: that is how the tests run it)
            peer = peer_exchange.create(self.group, index, peer_wait_s)
        self._direct, self.exchange_info = (peer_exchange.choose(self.group, be, rccl, peer, peer_wait_s)
                                            if (rccl or peer) else (None, {}))
        if self._direct is not None:
            self.exchange_info["route"] = getattr(self._direct, "route", "ncclAllGather on the detector's stream")
            ranks = getattr(self._direct, "comm_ranks", None)
            if ranks is not None:
                self.exchange_info["rccl_comm_ranks"] = ranks()  # ncclCommCount of the communicator the reports use
        if self.rank == 0:
            _LOG.info("straggler report exchange route: %s %s", self.exchange_info.get("route", "torch.distributed"),
                      {k: v for k, v in self.exchange_info.items() if k != "route"})

    def _exchange(self, be, ws):
        """The report's one collective: this rank's rows -> the [R, L] table, on the backend's stream."""
        if self._direct is not None:
            return self._direct.exchange(ws, be)
        with be.stream_context():  # the collective must queue behind the statistics kernel
            return dist_utils.all_gather_rows(ws.send, ws.table, self.group)

    def enqueue_only(self) -> bool:
        """Whether a steady-state ring report of this generator is only ENQUEUED (``asynchronous=True`` and nothing on the way
        needs the host: a single process, no exchange, or an in-stream exchange route).  On torch.distributed's route the
        collective is issued by the host between the two kernels and the report waits, whatever ``asynchronous`` says."""
        if not self.asynchronous:
            return False
        return self.world_size == 1 or not self._exchanged() or self._direct is not None or not self._direct_tried

    def take_unreported_rows(self) -> list:
        """Ring rows that held samples at the last ``generate_report_from_rings`` but were in no report (an asynchronous
        report that met a new name runs on the old tables): their samples belong to the next window.  Empty otherwise."""
        rows, self._unreported_rows = self._unreported_rows, []
        return rows

    def close(self) -> None:
        """Release the direct-exchange communicator (collective-free; safe to call more than once)."""
        # The remembered (default process group, group, (world, rank)) holds the ProcessGroup OBJECT.  A generator that outlives
        # destroy_process_group() would keep that object -- and gloo's worker threads, which its destructor joins -- alive
        # until the interpreter finalises; a worker that then releases the last tensor of its last collective asks for the GIL
        # of a finalising interpreter, CPython ends the thread with pthread_exit inside a noexcept C++ frame and the process
        # dies with "terminate called without an active exception" (the once-in-forty child abort of the reference's own
        # test_sections.py on a loaded host: profiles/r06_reftest_soak.txt has the native stack).
        self._wr_cache[0] = None
        if self._inflight is not None:
            try:
                self._settle_inflight()
            except Exception:  # noqa: BLE001  (shutdown path: a report that never completed must not mask it)
                self._inflight = None
        if self._direct is not None:
            self._direct.close()
            self._direct = None

    def _score_round(self, kernel_names: List[str], section_names: List[str], fill_send, local_ranks: int = 1,
                     stats_rows: int = 0, stats_rows_used: Optional[int] = None, sync_first: bool = False,
                     may_defer_sync: bool = False):
        """pack -> all-gather -> score, repeated once after a name sync if any rank met a new name.

        ``fill_send(ws, mapper, names_ok)`` must leave this rank's exchange rows in ``ws.send``.
        ``sync_first``: an earlier exchange already showed "ids missing" (``_take_resync``).  ``may_defer_sync``: a ring report
        that is not the generator's first -- one that meets ANOTHER rank's "ids missing" may have to leave the sync to the next.
        Returns ``(workspace, mapper)`` with the results in ``ws.scores / flags / meta / stats``.
        """
        be = _backend_mod.get_backend()
        exchanged = self._exchanged()
        mapper = self.name_mapper if exchanged else self._private_mapper
        if sync_first and exchanged and self.world_size > 1:
            # an exchange of this generator (the planned path's or the lane's, in this report or an asynchronous one before
            # it) carried an incomplete flag: every rank is now heading for the name sync, so join it before exchanging rows again.
            # (Only where rows ARE exchanged: a generator that scores this rank alone -- individual scores, no gather -- has
            # nobody heading anywhere; its own new names get their ids in the loop below.  An asynchronous generator of that
            # kind used to call the collective here, alone, the report after one of ITS sections first appeared: the rank hung
            # in all_gather_object while its peers trained on -- tools/soak_mp.py, profiles/r06af_soak_mp.txt.)
            mapper.sync_names(kernel_names, section_names)
        while True:
            names_ok = mapper.has_all_names(kernel_names, section_names)
            if not names_ok and (not exchanged or self.world_size == 1):
                self._assign_ids_locally(mapper, kernel_names, section_names)
                names_ok = True
            K, S = mapper.kernel_counter, mapper.section_counter
            world = self.world_size if exchanged else 1
            if self.work_groups:
                self._work_refuse(world * local_ranks)  # (before anything of this report is launched)
            ws = be.workspace(world * local_ranks, K, S, local_ranks, stats_rows)
            settle = getattr(ws, "settle_readers", None)  # (the CPU checker backend of the tests has no deferred readers)
            if settle is not None:
                settle()  # a follow-up kernel of the last report may still be reading the table that is about to be rewritten
            if world > 1:
                with be.stream_context():  # host-packed rows are copied on the stream the report runs on
                    fill_send(ws, mapper, names_ok)
                table = self._exchange(be, ws)
            else:
                fill_send(ws, mapper, names_ok)
                table = ws.send
            be.score(ws, table, self.is_computing_indiv_scores, self.is_computing_rel_scores, self.thresholds,
                     wait=True, stats_rows=stats_rows_used)
            if world > 1:
                self._check_exchange()
            if ws.meta[0] == 1:
                return ws, mapper
            if names_ok and world > 1 and may_defer_sync and self.enqueue_only():
                # Asynchronous reports on an in-stream route, and the names without ids are ANOTHER rank's: that rank only
                # enqueued this report (on its old tables, the flag in its row) and joins the name sync at the START of its next
                # report, when it settles this one -- it is not waiting inside this report, so neither a sync nor a second
                # exchange may happen here.  This rank got here because it left its cached plan in the very same report (its
                # occupied rows changed): it does what the planned path would have done -- keep the report, sync first next
                # time.  (It used to sync alone and exchange again: from then on its exchanges were paired with its peers'
                # NEXT ones, the last one with nobody -- tools/soak_mp.py, profiles/r06af_soak_mp.txt.)
                # (Not in a generator's FIRST ring report: no rank has a plan then, whoever flags is inside this report too.)
                # (The caller still ends by caching a plan for its new tables; the pending resync keeps it from ever running.)
                self._sync_names_first()
                return ws, mapper
            # some rank (maybe this one) has names without ids: cold path, then go again
            mapper.sync_names(kernel_names, section_names)

    # ---- report assembly --------------------------------------------------------------------------
    def _assemble(self, ws, mapper, local_section_names: Sequence[str], section_summaries, kernel_summaries,
                  t_start_ns: int, local_ranks: int = 1, stats: Optional[np.ndarray] = None):
        """Report of the general (name-syncing / dict-input) path.  ``section_summaries`` / ``kernel_summaries``
        are either the caller's dicts (handed on as they are, reporting.py:541-542) or name -> ring row
        tables to be resolved against ``stats``."""
        if self.gather_on_rank0 and self.rank != 0:
            return None
        rows = (section_summaries, kernel_summaries) if stats is not None else (None, None)
        view, lo, hi = self._view(ws, mapper, local_section_names, local_ranks, *rows)
        src = _ScoreSource(view)
        src.scores = ws.scores[lo:hi].copy()
        src.flags = ws.flags[lo:hi].copy()
        src.stats = stats
        report = Report._from_device(src, self._shared_rank_to_node(), (time.perf_counter_ns() - t_start_ns) * 1e-6,
                                     self.gather_on_rank0, self.rank)
        if self._table_steps_on:
            self._follow_ups(report, ws, mapper, view, lo, hi, None)
        if stats is None:
            # the caller's own summaries travel with the report, untouched
            report.__dict__["local_section_summaries"] = section_summaries
            report.__dict__["local_kernel_summaries"] = kernel_summaries
        return report

    def _view(self, ws, mapper, local_section_names: Sequence[str], local_ranks: int, section_rows, kernel_rows,
              stats_needed: Optional[int] = None):
        """What a report shows of the table in ``ws``: rank 0 of a gathering generator sees every rank's rows and every section
        that has an id, any other generator its own rows and its own sections.  Returns ``(view, first row, end row)``.
        ``stats_needed`` (a plan's reports, read lazily from the result block): also where those rows sit in the block."""
        if self.gather_on_rank0:
            lo, hi = 0, ws.R
            ranks = range(ws.R)
            names = [mapper.get_section_name(i) for i in range(ws.S)]
        else:
            lo = self.rank * local_ranks if self._exchanged() else 0
            hi = lo + local_ranks
            ranks = range(self.rank * local_ranks, (self.rank + 1) * local_ranks)
            names = list(local_section_names)
        v = _View()
        v.S, v.ranks, v.names, v.cols = ws.S, ranks, names, {n: mapper.get_section_id(n) for n in names}
        v.has_rel, v.has_indiv = self.is_computing_rel_scores, self.is_computing_indiv_scores
        v.section_rows, v.kernel_rows = section_rows, kernel_rows
        v.layout = None if stats_needed is None else (ws._off_scores, ws._off_flags, ws._off_stats, ws.R, ws.W, lo, hi, stats_needed)
        v.thresholds = self.thresholds
        return v, lo, hi

    @staticmethod
    def _assign_ids_locally(mapper, kernel_names, section_names) -> None:
        """Nobody to agree with (one rank, or a generator that exchanges nothing): extend the tables locally, in the order a
        1-rank name sync would."""
        for s in section_names:
            mapper._assign_section_id(s)
        for k in kernel_names:
            mapper._assign_kernel_id(k)

    @staticmethod
    def _point_ring_rows(rings, mapper, ws) -> None:
        """Point every ring row at its slot of the exchange row (cold: ids or workspace changed)."""
        for name, row in rings.kernel_row_names.items():
            g = mapper.kernel_name_to_id.get(name, -1) if not is_collective_kernel(name) else -1
            rings.configure(row, 1, g)
        for name, row in rings.section_row_names.items():
            g = mapper.section_name_to_id.get(name)
            rings.configure(row, 0, ws.K + g if g is not None else -1)
        ws.send_initialised = False

    # ---- steady-state plan of the ring path ---------------------------------------------------------
    class _RingPlan:
        """Everything about a ring report that only changes when names, ids or topology change."""

        __slots__ = ("key", "topology", "ws", "mapper", "rows_used", "stats_needed", "section_rows", "kernel_rows", "fused", "view")

    def _plan_key(self, rings, section_rows, kernel_rows, local_ranks):
        """A cached plan serves a report whose key equals the plan's: same name tables (the caller hands the same dicts while
        the occupied rows stay the same), same ids, same topology."""
        return (id(section_rows), len(section_rows), id(kernel_rows), len(kernel_rows), self.name_mapper.version,
                self._private_mapper.version, self.world_size, self.rank, rings.rows_used, local_ranks, id(rings))

    def _plan_topology(self, rings, local_ranks):
        """What names and ids have no say in (cold; kept on the plan: the asynchronous "new name" branch asks whether it still holds)."""
        return (self.world_size, self.rank, local_ranks, id(rings))

    def _build_ring_plan(self, key, rings, section_rows, kernel_rows, local_ranks):
        be = _backend_mod.get_backend()
        exchanged = self._exchanged()
        mapper = self.name_mapper if exchanged else self._private_mapper
        knames, snames = list(kernel_rows.keys()), list(section_rows.keys())
        if not mapper.has_all_names(knames, snames):
            if exchanged and self.world_size > 1:
                return None  # ids must be agreed with the other ranks first: general path
            self._assign_ids_locally(mapper, knames, snames)
        K, S = mapper.kernel_counter, mapper.section_counter
        world = self.world_size if exchanged else 1
        total_rows = rings.local_ranks * rings.rows_per_rank
        plan = self._RingPlan()
        plan.key = key
        plan.topology = self._plan_topology(rings, local_ranks)
        plan.mapper = mapper
        if self.work_groups:
            self._work_refuse(world * local_ranks)
        plan.ws = be.workspace(world * local_ranks, K, S, local_ranks, total_rows)
        plan.rows_used = rings.rows_used
        # the report's local summaries are those of this process' FIRST logical rank (rank 0 of a folded job): its rows are
        # the first rows_used statistics rows, whatever the number of logical ranks -- nothing else is forwarded or copied
        plan.stats_needed = rings.rows_used
        plan.section_rows, plan.kernel_rows = section_rows, kernel_rows
        plan.fused = hasattr(rings, "report_fused")  # the HIP engine; the CPU test backend takes the stepwise route
        self._point_ring_rows(rings, mapper, plan.ws)
        # the part of a report that every report of the plan shares (built once per plan)
        plan.view = self._view(plan.ws, mapper, snames, local_ranks, section_rows, kernel_rows, plan.stats_needed)[0]
        self._ring_gid_state = None  # the general path must re-derive its own view if it runs next
        return plan

    # ---- name-sync and in-flight state: every transition of DESIGN.md section 4's table, once -------------
    def _settle_inflight(self) -> bool:
        """Wait for the asynchronous report still in flight (if any) before its workspace is touched again.
        Returns True when that report's exchange showed a rank with names that have no id yet: every rank sees the
        same table, so every rank learns it here, at the same point of the program, and goes through the name sync
        (the caller says so with ``_sync_names_first``; the dict-input path checks names in its score round anyway)."""
        pend = self._inflight
        if pend is None:
            return False
        self._inflight = None
        names_word = pend.complete()  # a poll; the block is copied only if / when somebody reads or outlives it
        self._prev_async_settled = True  # observed, not assumed: the next report tells the library so (prev_settled)
        self._check_exchange()
        return names_word != 1

    def _drop_plan(self) -> None:
        """The cached plan never runs again (a planned or lane report raised: e.g. a timed-out wait retired its workspace)."""
        self._ring_plan = None

    def _sync_names_first(self) -> None:
        """Some rank's table said "ids missing": every rank is heading for the name sync, at the start of its next pass
        through the general path -- in this very ``generate_report_from_rings`` call when a settled or synchronous report
        showed it.  Until then neither a cached plan nor Detector's lane runs."""
        self._ring_plan = None
        self._resync_pending = True

    def _take_resync(self) -> bool:
        """The general path of a ring report, about to enter its score round: whether that starts with the name sync."""
        pending, self._resync_pending = self._resync_pending, False
        return pending

    def _check_exchange(self) -> None:
        check = getattr(self._direct, "check", None)  # the peer-window route reports peers that never arrived
        if check is not None:
            check()

    def _report_from_plan(self, plan, rings, t0, order_after=None, names_ok: bool = True, reset_rings: bool = False):
        """The steady-state report: ONE C call (statistics kernel, the collective, score kernel, wait), one host
        copy of the result block, mappings built on first read.  Asynchronous generators only enqueue.  A synchronous
        report without an exchange is issued and waited for in two calls where the rings can, with the Report built in
        between (``_report_split``)."""
        be = _backend_mod.get_backend()
        ws = plan.ws
        multi = self.world_size > 1 and self._exchanged()
        fused = plan.fused and (not multi or self._direct is not None)
        follow_ups = self._table_steps_on
        settle = getattr(ws, "settle_readers", None)  # (the CPU checker backend of the tests has no deferred readers)
        if settle is not None:
            settle()  # a follow-up kernel of the last report may still be reading the table that is about to be rewritten
        self._last_plan_fused = fused
        if follow_ups and fused:
            for option, method in self._one_call_needs:  # (before anything of this report is issued)
                if not hasattr(rings, method):
                    raise RuntimeError(f"{option}: these rings run the one-call report but have no {method}")
        if fused:
            # ONE C call: flush -> statistics kernel -> [ncclAllGather] -> score kernel -> completion word
            wait = not self.asynchronous
            if wait and not multi and self._report_split:
                issue = getattr(rings, "report_issue", None)  # (the CPU checker backends of the tests have the one call only)
                if issue is not None:
                    return self._report_split_from_plan(plan, rings, be, t0, issue, names_ok, reset_rings)
            seq = rings.report_fused(ws, plan.rows_used, plan.stats_needed, self.is_computing_indiv_scores,
                                     self.is_computing_rel_scores, self.thresholds, self._direct if multi else None,
                                     names_ok=names_ok, wait=wait, order_after=order_after if multi else None,
                                     resident=not (multi and getattr(self._direct, "shared_device", False)
                                                   and os.environ.get("NVRX_DEBUG_RESIDENT_SHARED_OK", "0") in ("", "0")),
                                     prev_settled=self._prev_async_settled)
            if not wait:
                # the report is only enqueued (the lane's hot path mirrors these two writes: straggler._Lane.run)
                self._prev_async_settled = False  # until somebody has seen THIS report complete
                pend = self._inflight = _PendingBlock(be, ws, seq)
                if self.gather_on_rank0 and self.rank != 0:
                    return None
                report = Report._from_device(
                    _ScoreSource(plan.view, pend),
                    self._shared_rank_to_node(),
                    (time.perf_counter_ns() - t0) * 1e-6, self.gather_on_rank0, self.rank)
                if follow_ups:
                    view = plan.view
                    self._follow_ups(report, ws, plan.mapper, view, view.layout[5], view.layout[6], rings)
                return report
        else:
            rings.report_local(ws, True, rows_active=plan.rows_used)
            table = self._exchange(be, ws) if multi else ws.send
            be.score(ws, table, self.is_computing_indiv_scores, self.is_computing_rel_scores, self.thresholds,
                     wait=True, stats_rows=plan.stats_needed)
        if fused:
            # a resident score kernel forwards the statistics rows AFTER the scores: whatever this call returns or
            # raises, the next user of the workspace must see them landed (meta[5]) before it enqueues anything that
            # writes them
            mark = getattr(ws, "mark_live", None)  # (the CPU checker backend of the tests has no deferred rows)
            if mark is not None:
                mark(ws.seq)
        if multi:
            self._check_exchange()  # a peer that never arrived: this report's scores are invalid, the next one is not
        if ws.meta[0] != 1:
            return False  # another rank met a new name: fall back to the general (name-syncing) path
        if self.gather_on_rank0 and self.rank != 0:
            return None
        if fused:
            # nothing is copied now: scores / flags / statistics leave the block when the report is first read, or when
            # the workspace is about to be reused and the report is still held
            pending = _LiveBlock(be, ws, ws.seq, plan.stats_needed)
            ws.attach(pending)  # the workspace collects it (if still held) before the block is reused by anybody
        else:
            pending = ws.host_block()
        report = Report._from_device(
            _ScoreSource(plan.view, pending),
            self._shared_rank_to_node(),
            (time.perf_counter_ns() - t0) * 1e-6, self.gather_on_rank0, self.rank)
        if follow_ups:
            view = plan.view
            self._follow_ups(report, ws, plan.mapper, view, view.layout[5], view.layout[6], rings if fused else None)
        return report

    def _report_split_from_plan(self, plan, rings, be, t0, issue, names_ok: bool, reset_rings: bool):
        """``_report_from_plan`` for a synchronous one-call report of a single process, in two C calls: issue (both launches),
        build on the host what needs none of the results -- the live block, the Report, the emptied rings -- while the GPU
        runs, wait, look at ``meta[0]``.  Every way out leaves what the one-call path leaves: a wait that raises leaves the
        block nobody's (``rings.report_wait``) and the caller drops the plan; "ids missing" leaves it as ``mark_live`` does.
        The follow-up kernels of the per-report options are enqueued behind the wait, where the one-call path enqueues them:
        the library takes the completion word as proof that its stream has drained, which holds for nothing enqueued
        in between."""
        ws = plan.ws
        seq = issue(ws, plan.rows_used, plan.stats_needed, self.is_computing_indiv_scores, self.is_computing_rel_scores,
                    self.thresholds, None, names_ok=names_ok, order_after=None, resident=True)
        report = None
        if not (self.gather_on_rank0 and self.rank != 0):
            pending = _LiveBlock(be, ws, seq, plan.stats_needed)
            ws.attach(pending)  # the workspace collects it (if still held) before the block is reused by anybody
            report = Report._from_device(_ScoreSource(plan.view, pending), self._shared_rank_to_node(), 0.0,
                                         self.gather_on_rank0, self.rank)
        if reset_rings and not self._ring_steps_on:
            # the statistics kernel has its counts (include/nvrx_straggler.h, nvrx_ring_reset); the steps that read the
            # rings again after the report -- row families, slack -- are off, and so is the general path: "ids missing" comes
            # out of another process' row or out of names_ok=False, which only an asynchronous report passes
            rings.reset()
            self._rings_were_reset = True
        rings.report_wait(ws)
        if report is None or ws.meta[0] != 1:
            mark = getattr(ws, "mark_live", None)
            if mark is not None:
                mark(seq)  # nobody holds this report: the block's next user still has to see its statistics rows land
            if ws.meta[0] != 1:
                return False  # (a name without an id: the general path; the Report built above is let go here)
            return None
        report.__dict__["generate_report_elapsed_time"] = (time.perf_counter_ns() - t0) * 1e-6
        if self._table_steps_on:
            view = plan.view
            self._follow_ups(report, ws, plan.mapper, view, view.layout[5], view.layout[6], rings)
        return report

    # ---- the table follow-ups of a report: every route's, in the one order ----------------------------
    def _follow_ups(self, report, ws, mapper, view, lo: int, hi: int, rings) -> None:
        """Enqueue every table follow-up that is switched on behind the report that was just issued on ``ws``, for the ranks
        ``[lo, hi)`` it covers, and hang each on ``report`` unread.  Nothing is waited for (but ``peer_groups="auto"``: its
        groups are the work step's records).  ``rings``: the one-call report's rings, whose ``report_<x>`` entries the library
        orders behind that report's kernels; None: the backend's stepwise entries on ``ws.table``, behind the score kernel on
        the backend's stream.  The order below is the contract ("The follow-ups' order"): ``settle_readers``
        delivers in it, the peer step needs the work step's handle, the histories run directly behind what they record."""
        be, d, n = _backend_mod.get_backend(), report.__dict__, hi - lo
        if self.kernel_attribution:
            if rings is not None:
                handle = rings.report_attribute(ws, self.kernel_attribution, lo, n)
            else:
                handle = be.attribute(ws, ws.table, self.kernel_attribution, self.is_computing_indiv_scores,
                                      self.is_computing_rel_scores, lo, n)
            d["_attr"] = self._attr_source(handle, ws, mapper, lo, hi, view.ranks)
        if self.robust_scores:
            least = self._robust_min(ws)
            if rings is not None:
                handle = rings.report_robust(ws, lo, n, least, self.robust_floor)
            else:
                handle = be.robust_score(ws, ws.table, lo, n, least, self.robust_floor)
            d["_robust"] = _RobustSource(handle, view.ranks, view.cols, self._attr_names(mapper, ws.K), least, self.robust_floor)
        if self.work_groups:
            # all R ranks (the components need them); ahead of the peer step, which peer_groups="auto" makes wait for it
            if rings is not None:
                handle = rings.report_work(ws, self.work_count_tol, self.work_max_unlike_ppm)
            else:
                handle = be.work_groups(ws, ws.table, self.work_count_tol, self.work_max_unlike_ppm)
            self._work_handle = handle  # (before anything of this report asks _peer_for)
            labelled = self._peer_for(ws) if self.peer_groups is not None and self.peer_groups != "auto" else None
            d["_work"] = _WorkSource(handle, view.ranks, {"count_tol": self.work_count_tol, "max_unlike": self.work_max_unlike,
                                                          "max_unlike_ppm": self.work_max_unlike_ppm}, labelled)
        if self.peer_groups is not None:
            groups = self._peer_for(ws)
            if rings is not None:
                peer = rings.report_peer(ws, groups, lo, n, self.peer_min_ranks)
            else:
                peer = be.peer_score(ws, ws.table, groups, lo, n, self.peer_min_ranks)
            d["_peer"] = _PeerSource(peer, view.ranks, view.cols, self._attr_names(mapper, ws.K), groups, self.peer_min_ranks)
            if self._peer_history is not None:
                # directly behind the peer step, on the stream it used, once per report for which that step ran on this rank
                # and never otherwise: that is what the history's n_before counts
                state, thr = self._peer_history, self.peer_persistence_thresholds
                if rings is not None:
                    handle = rings.report_peer_history(ws, state, peer, thr)
                else:
                    handle = be.peer_history(ws, state, peer, thr)
                d["_peer_history"] = _PeerHistorySource(handle, view.ranks, view.cols, self.peer_history,
                                                        self.peer_persistence_min_reports, thr)
                if self.peer_trends:
                    handle = rings.report_peer_trend(ws, state) if rings is not None else be.peer_trend(ws, state)
                    d["_peer_trends"] = _PeerTrendSource(handle, view.ranks, view.cols, min(state.n_before, self.peer_history),
                                                         self.trend_min_reports, self.trend_min_tau, self.peer_trend_horizon, thr)
        if self.pace_scores:
            least = self._pace_min(ws)
            params = {"min_ranks": least, "min_columns": self.pace_min_columns, "min_effect": self.pace_min_effect,
                      "min_breadth": self.pace_min_breadth}
            if self.pace_peer_groups:
                groups = self._peer_for(ws)
                if rings is not None:
                    handle = rings.report_pace_group(ws, groups, lo, n, least, self.peer_min_ranks)
                else:
                    handle = be.pace_group_score(ws, ws.table, groups, lo, n, least, self.peer_min_ranks)
                params.update(min_peers=self.peer_min_ranks, peer_groups=True)
                d["_pace"] = _PaceGroupSource(handle, view.ranks, view.cols, self._attr_names(mapper, ws.K), params, groups)
            else:
                handle = rings.report_pace(ws, lo, n, least) if rings is not None else be.pace_score(ws, ws.table, lo, n, least)
                d["_pace"] = _PaceSource(handle, view.ranks, view.cols, self._attr_names(mapper, ws.K), params)
        if self.node_scores:
            nodes = self._node_for(ws)
            least = self._node_min(nodes)
            if rings is not None:
                handle = rings.report_node(ws, nodes, lo, n, self.node_min_members, least)
            else:
                handle = be.node_score(ws, ws.table, nodes, lo, n, self.node_min_members, least)
            params = {"min_members": self.node_min_members, "min_nodes": least, "min_columns": self.node_min_columns,
                      "min_effect": self.node_min_effect, "min_breadth": self.node_min_breadth, "min_agree": self.node_min_agree}
            d["_node"] = _NodeSource(handle, view.ranks, view.cols, self._attr_names(mapper, ws.K), params, nodes)
        if self._history is not None:
            # the ring takes the scores of every report this rank holds, once, behind its last score kernel
            state, thr = self._history, self.persistence_thresholds
            if rings is not None:
                handle = rings.report_history(ws, state, lo, n, thr)
            else:
                handle = be.score_history(ws, state, lo, n, thr)
            d["_history"] = _HistorySource(handle, view.ranks, view.cols, self.is_computing_rel_scores,
                                           self.is_computing_indiv_scores, self.score_history, self.persistence_min_reports, thr)
            if self.score_trends:
                # ... and the trends of the ring as that step leaves it, behind it
                handle = rings.report_trend(ws, state) if rings is not None else be.score_trend(ws, state)
                d["_trends"] = _TrendSource(handle, view.ranks, view.cols, self.is_computing_rel_scores,
                                            self.is_computing_indiv_scores, min(state.n_before, self.score_history),
                                            self.trend_min_reports, self.trend_min_tau, self.trend_horizon, thr)

    # ---- robust scores ------------------------------------------------------------------------------
    def _robust_min(self, ws) -> int:
        """``robust_min_ranks``, but never more than the ranks the table has: a job smaller than that is rated against its own
        median all the same (one rank: ratio 1, z 0)."""
        return min(self.robust_min_ranks, ws.R)

    # ---- peer-group scores --------------------------------------------------------------------------
    def _peer_for(self, ws):
        """The groups resolved for the logical ranks of ``ws``' table (cold: once per R; a label list of another length
        is refused here, where R is first known)."""
        groups = self._peer_resolved
        if self.peer_groups == "auto":
            # the work groups of THIS report's table: one stream wait and one D2H of the rank records and the job record (an
            # asynchronous report waits here too); the roots are the labels, and the object is kept while they stay the same
            rec, _ = self._work_handle.records()
            roots = np.ascontiguousarray(rec[:, 0], dtype=np.uint32).view(np.int32)
            if groups is None or groups.R != ws.R or not np.array_equal(roots, self._peer_auto_roots):
                groups = self._peer_resolved = _backend_mod.PeerGroups(roots.tolist())
                self._peer_auto_roots = roots.copy()
            return groups
        if groups is None or groups.R != ws.R:
            groups = self._peer_resolved = _backend_mod.PeerGroups.resolve(self.peer_groups, ws.R)
        return groups

    # ---- work groups --------------------------------------------------------------------------------
    def _work_refuse(self, R: int) -> None:
        """The step compares every pair of ranks and takes at most ``NVRX_WORK_MAX_RANKS`` of them."""
        cap = _backend_mod._native.WORK_MAX_RANKS
        if R > cap:
            option = "peer_groups='auto'" if self.peer_groups == "auto" else "work_groups"
            raise ValueError(f"{option}: the job has {R} logical ranks, work groups are inferred for at most {cap}; say which "
                             "ranks do the same work with peer_groups labels, 'block:N' or 'mod:N' instead")

    # ---- pace scores --------------------------------------------------------------------------------
    def _pace_min(self, ws) -> int:
        """``pace_min_ranks``, but never more than the ranks the table has, as ``_robust_min``."""
        return min(self.pace_min_ranks, ws.R)

    # ---- node scores --------------------------------------------------------------------------------
    def _node_for(self, ws):
        """The nodes resolved for the logical ranks of ``ws``' table (cold: once per R and, with ``node_groups=None``, per
        ``rank_to_node`` -- a plain dict that is replaced, never edited, when it changes; a label list of another length is
        refused here, where R is first known).  No collective: ``rank_to_node`` is what the name sync gathered."""
        nodes = self._node_resolved
        if self.node_groups is not None:
            if nodes is None or nodes.R != ws.R:
                nodes = self._node_resolved = _backend_mod.PeerGroups.resolve(self.node_groups, ws.R, "node_groups")
            return nodes
        r2n = self.rank_to_node
        if nodes is None or nodes.R != ws.R or self._node_source is not r2n:
            missing = [r for r in range(ws.R) if r not in r2n]
            if missing:
                raise ValueError(f"node_scores: rank_to_node names {len(r2n)} of the job's {ws.R} logical ranks (it is gathered "
                                 f"with gather_on_rank0=True; rank {missing[0]} is missing); pass node_groups "
                                 "('block:N', 'mod:N' or one label per logical rank)")
            nodes = self._node_resolved = _backend_mod.PeerGroups([r2n[r] for r in range(ws.R)])
            self._node_source = r2n
        return nodes

    def _node_min(self, nodes) -> int:
        """``node_min_nodes``, but never more than the nodes the job has, as ``_pace_min``."""
        return min(self.node_min_nodes, nodes.G)

    # ---- score history ------------------------------------------------------------------------------
    def reset_score_history(self) -> None:
        """Forget the score history: the next report starts a new one (after a restart from a checkpoint, a change of the
        job's layout, a node swap) -- and so does the peer-score history.  Reports already handed out keep theirs."""
        if self._history is not None:
            self._history.reset()
        if self._peer_history is not None:
            self._peer_history.reset()

    # ---- row families: tail, onset, period, episode scores ------------------------------------------
    def _family_step(self, fam, report, rings, ws, mapper, rows_active: int, fused: bool, local_ranks: int) -> None:
        """One row family's step of a ring report, once per ``generate_report_from_rings`` call behind its last score round
        (and behind the steps of the families before it), on that round's workspace: the family's ring kernel on the window
        the report saw -> [one all-gather of its rows] -> its score kernel for the ranks the report covers, hung on ``report``
        unread.  Every rank issues it at every report, whatever the report found and whether or not it holds a report (a
        gathering generator's other ranks): same collectives everywhere."""
        be = _backend_mod.get_backend()
        params = fam.params(self)
        local, score = getattr(rings, fam.name + "_local", None), getattr(be, fam.name + "_score", None)
        if local is None or score is None:
            raise RuntimeError(f"{fam.label(params)}: the active backend has no {fam.name} scores "
                               f"(rings.{fam.name}_local / backend.{fam.name}_score)")
        table = self._gather_step_rows(be, *local(ws, *params, rows_active, fused))
        if report is None or report is False:
            return
        lo, hi = self._covered(ws, local_ranks)
        view = report.__dict__["_src"].view
        if self.row_peer_groups:
            grouped = getattr(be, fam.name + "_group_score", None)
            if grouped is None:
                raise RuntimeError(f"row_peer_groups: the active backend has no {fam.name} scores per peer group "
                                   f"(backend.{fam.name}_group_score)")
            groups = self._peer_for(ws)  # (with "auto": the work groups of this report, whose step has run by now)
            handle = grouped(ws, table, ws.table, groups, lo, hi - lo, self.peer_min_ranks, *params[:fam.score_params])
            report.__dict__[fam.slot] = _RowGroupFamilySource(fam, handle, view.ranks, view.cols,
                                                              self._attr_names(mapper, ws.K), params, groups, self.peer_min_ranks)
            return
        handle = score(ws, table, ws.table, lo, hi - lo, *params[:fam.score_params])
        report.__dict__[fam.slot] = _RowFamilySource(fam, handle, view.ranks, view.cols, self._attr_names(mapper, ws.K), params)

    def _ring_steps(self, report, rings, ws, mapper, rows_active: int, fused: bool, local_ranks: int) -> None:
        """The ring steps of one ``generate_report_from_rings`` call: the families that are switched on, in the table's order,
        then slack -- the order of their collectives, the same on every rank whatever ``report`` is."""
        if not self._ring_steps_on:
            return
        for fam in self._row_families:
            self._family_step(fam, report, rings, ws, mapper, rows_active, fused, local_ranks)
        if self.collective_slack:
            self._slack_step(report, rings, ws, rows_active, fused, local_ranks)

    def _gather_step_rows(self, be, send, table):
        """Exchange a ring step's rows behind its local kernel: its one collective, on the backend's stream."""
        if self.world_size > 1:
            with be.stream_context():
                table = dist_utils.all_gather_rows(send, table, self.group)
        return table

    def _covered(self, ws, local_ranks: int):
        """The ranks ``[lo, hi)`` a ring step scores for the report this rank holds.  (Not ``_view``'s rule: a step's table
        is exchanged whether or not the report's is, so this rank's rows always sit at ``rank * local_ranks``.)"""
        if self.gather_on_rank0:
            return 0, ws.R
        lo = self.rank * local_ranks
        return lo, lo + local_ranks

    # ---- slack scores -------------------------------------------------------------------------------
    def _slack_step(self, report, rings, ws, rows_active: int, fused: bool, local_ranks: int) -> None:
        """The slack step of a ring report, once per ``generate_report_from_rings`` call right behind the row families'
        steps, on the same workspace: the local kernel on the statistics the report wrote (the collective kernels' rows, which
        the report itself does not exchange) -> [one all-gather of its rows] -> the score kernels, hung on ``report`` unread.
        Like a family's step, every rank issues it at every report, whatever the report found and whether or not it holds a
        report: same collectives everywhere."""
        be = _backend_mod.get_backend()
        local, score = getattr(rings, "slack_local", None), getattr(be, "slack_score", None)
        if local is None or score is None or not hasattr(rings, "slack_list"):
            raise RuntimeError("collective_slack: the active backend has no slack scores (rings.slack_local, rings.slack_list / "
                               "backend.slack_score)")
        table = self._gather_step_rows(be, *local(ws, rows_active, fused))
        if report is None or report is False:
            return
        lo, hi = self._covered(ws, local_ranks)
        view = report.__dict__["_src"].view
        if self.slack_peer_groups:
            grouped = getattr(be, "slack_group_score", None)
            if grouped is None:
                raise RuntimeError("slack_peer_groups: the active backend has no slack scores per peer group "
                                   "(backend.slack_group_score)")
            groups = self._peer_for(ws)  # (with "auto": the work groups of this report, whose step has run by now)
            handle = grouped(ws, table, ws.table, groups, lo, hi - lo, self.slack_min_ranks, self.peer_min_ranks)
            report.__dict__["_slack"] = _SlackGroupSource(handle, view.ranks, rings.slack_list()[2], groups, self.slack_min_ranks,
                                                          self.peer_min_ranks, self.slack_min_share, self.slack_max_ratio)
            return
        min_ranks = min(self.slack_min_ranks, ws.R)
        handle = score(ws, table, ws.table, lo, hi - lo, min_ranks)
        report.__dict__["_slack"] = _SlackSource(handle, view.ranks, rings.slack_list()[2], min_ranks, self.slack_min_share,
                                                 self.slack_max_ratio)

    # ---- public: summaries given as dicts (reference signature) -------------------------------------
    def generate_report(self, section_summaries: Mapping[str, _SummaryType],
                        kernel_summaries: Mapping[str, _SummaryType]):
        """Score the given per-rank summaries (name -> {Statistic: value}).

        Collective.  Returns a :class:`Report`, or ``None`` on ranks other than 0 when
        ``gather_on_rank0`` is set.  The summaries are packed into this rank's exchange row on the
        host; exchange and scoring run on the device exactly as in the ring path.  Summaries hold no samples: a report
        of this path carries no tail scores (``tail_quantile``; ``Report.tail_scores()`` is ``{}``), no onset scores
        (``onset_detection``; ``Report.onset_scores()`` is ``{}``), no period scores (``period_detection``;
        ``Report.period_scores()`` is ``{}``) and no episode scores (``episode_detection``; ``Report.episode_scores()`` is
        ``{}``).
        """
        t0 = time.perf_counter_ns()
        self.world_size = dist_utils.get_world_size(self.group)
        self.rank = dist_utils.get_rank(self.group)
        if self._inflight is not None:
            self._settle_inflight()  # ("ids missing" in that report's table is not acted on: the score round below checks names anyway)
        if not self._direct_tried:
            self._maybe_create_direct_exchange()
        kernel_summaries = self._filter_out_nccl_kernels(kernel_summaries)
        self._maybe_gather_rank_to_node()
        if self.is_computing_indiv_scores:
            self._update_local_min_times(kernel_summaries, section_summaries)
        knames, snames = list(kernel_summaries.keys()), list(section_summaries.keys())

        def fill_send(ws, mapper, names_ok):
            K, KS, L = ws.K, ws.K + ws.S, ws.L
            row = np.zeros(L, dtype=np.float32)
            row[:KS] = -1.0
            row[KS : 2 * KS] = np.nan
            for name, summ in kernel_summaries.items():
                g = mapper.kernel_name_to_id.get(name)
                if g is None:
                    continue  # no id yet: this round only carries the "names incomplete" flag
                row[g] = summ[Statistic.MED]
                row[KS + g] = self.min_local_kernel_times[name] if self.is_computing_indiv_scores else np.nan
                row[2 * KS + g] = summ[Statistic.NUM] * summ[Statistic.AVG]
            for name, summ in section_summaries.items():
                g = mapper.section_name_to_id.get(name)
                if g is None:
                    continue
                row[K + g] = summ[Statistic.MED]
                row[KS + K + g] = self.min_local_section_times[name] if self.is_computing_indiv_scores else np.nan
            row[L - 1] = 1.0 if names_ok else 0.0
            ws.set_send_row(0, row)

        ws, mapper = self._score_round(knames, snames, fill_send)
        return self._assemble(ws, mapper, snames, section_summaries, kernel_summaries, t0)

    # ---- internal: summaries never leave the device (Detector path) -----------------------------------
    def generate_report_from_rings(self, rings, section_rows: Mapping[str, int], kernel_rows: Mapping[str, int],
                                   local_ranks: int = 1, order_after: Optional[int] = None, reset_rings: bool = False):
        """Report straight from the device rings: statistics kernel -> exchange -> score kernel.

        ``section_rows`` / ``kernel_rows`` map the names that hold samples this window to their ring
        rows.  Replaces ``_get_section_summaries`` + ``_get_kernel_summaries`` + ``generate_report``
        of the reference (straggler.py:236-239) without materialising per-section Python objects.
        ``order_after``: raw ``hipStream_t`` of the caller's current stream; a multi-rank report is ordered after the
        work already enqueued there (the collectives of the training step) on the device, without a host wait.
        ``reset_rings``: empty the rings (``rings.reset()``) once the report has what it needs of them -- while the GPU
        runs, where the report is issued and waited for in two calls; before returning, on every other path.
        """
        t0 = time.perf_counter_ns()
        self.world_size, self.rank = dist_utils.world_and_rank(self.group, self._wr_cache)
        if self._starts_family is not None and not getattr(rings, "onset_enabled", False):
            if not hasattr(rings, "onset_enable"):
                raise RuntimeError(f"{self._starts_family.option}: the active backend has no ring-start snapshot (rings.onset_enable)")
            rings.onset_enable(True)  # (before this window's report: it notes where every ring's oldest sample lives)
        if not self._direct_tried and self.world_size != 1:  # (a single process has no route to build)
            self._maybe_create_direct_exchange()
        if self._inflight is not None and self._settle_inflight():
            # the previous (asynchronous) report's exchange carried an "ids missing" flag: every rank is here now
            self._sync_names_first()
        if self._resync_pending:
            # every rank is heading for the name sync: no cached plan runs before it -- neither the one dropped when the flag
            # was seen nor the one that the report which DEFERRED its sync (see _score_round) cached on its way out
            self._ring_plan = None
        # steady state: same name tables as last time -> run the cached plan
        plan = self._ring_plan
        if plan is not None and plan.key == self._plan_key(rings, section_rows, kernel_rows, local_ranks):
            try:
                out = self._report_from_plan(plan, rings, t0, order_after, True, reset_rings)
            except Exception:
                self._rings_were_reset = False
                self._drop_plan()
                raise
            if out is not False:
                self._ring_steps(out, rings, plan.ws, plan.mapper, plan.rows_used, self._last_plan_fused, local_ranks)
                if reset_rings:
                    if self._rings_were_reset:
                        self._rings_were_reset = False
                    else:
                        rings.reset()
                return out
            self._rings_were_reset = False  # (the general path below empties them at its end)
            self._sync_names_first()  # some OTHER rank met a new name during this report's exchange
        elif (plan is not None and self.enqueue_only() and plan.fused and plan.topology == self._plan_topology(rings, local_ranks)
              and not plan.mapper.has_all_names(list(kernel_rows.keys()), list(section_rows.keys()))):
            # asynchronous + a name this rank has no id for: the other ranks will not wait inside this report, so the
            # name exchange cannot happen now.  Run the OLD plan (the new rows are not exchanged yet) with the
            # "ids missing" flag in this rank's row; every rank meets it when it settles this report and they all
            # sync names at the start of the next one.  The rows of the new names are in nobody's report this time: the caller
            # keeps their samples for the next window instead of dropping them with the rest (take_unreported_rows).
            known_k, known_s = plan.kernel_rows, plan.section_rows
            self._unreported_rows = ([r for n, r in kernel_rows.items() if n not in known_k and not is_collective_kernel(n)]
                                     + [r for n, r in section_rows.items() if n not in known_s])
            out = self._report_from_plan(plan, rings, t0, order_after, names_ok=False)
            self._ring_steps(out, rings, plan.ws, plan.mapper, plan.rows_used, self._last_plan_fused, local_ranks)
            if reset_rings:
                rings.reset()
            return out
        kernel_rows = {k: r for k, r in kernel_rows.items() if not is_collective_kernel(k)} if any(
            is_collective_kernel(k) for k in kernel_rows) else kernel_rows
        self._maybe_gather_rank_to_node()
        if local_ranks > 1 and not self._rank_to_node_folded:
            # folded runs: every logical rank inherits the node of the process that holds it
            per_proc = dict(self.rank_to_node)
            self.rank_to_node = {p * local_ranks + q: node for p, node in per_proc.items() for q in range(local_ranks)}
            self._rank_to_node_folded = True
        knames, snames = list(kernel_rows.keys()), list(section_rows.keys())
        rows_used = rings.rows_used
        total_rows = rings.local_ranks * rings.rows_per_rank
        stats_needed = rows_used  # (see _build_ring_plan)

        def fill_send(ws, mapper, names_ok):
            state = (id(mapper), mapper.version, rows_used, id(ws))
            if self._ring_gid_state != state:
                self._point_ring_rows(rings, mapper, ws)  # (ids changed)
                self._ring_gid_state = state
            rings.report_local(ws, names_ok, rows_active=rows_used)

        not_the_first, self._had_ring_report = self._had_ring_report, True
        ws, mapper = self._score_round(knames, snames, fill_send, local_ranks=local_ranks, stats_rows=total_rows,
                                       stats_rows_used=stats_needed, sync_first=self._take_resync(), may_defer_sync=not_the_first)
        report = self._assemble(ws, mapper, snames, dict(section_rows), dict(kernel_rows), t0, local_ranks=local_ranks,
                                stats=ws.stats[:stats_needed].copy())
        # before the plan below re-points the ring rows (the slack step's list is built from the rings' own table of kernel
        # rows: the collective ones were filtered out of kernel_rows above)
        self._ring_steps(report, rings, ws, mapper, rows_used, False, local_ranks)
        # names are settled now: the next report with the same tables takes the planned path
        self._ring_plan = self._build_ring_plan(self._plan_key(rings, section_rows, kernel_rows, local_ranks), rings,
                                                section_rows, kernel_rows, local_ranks)
        if reset_rings:
            rings.reset()
        return report
