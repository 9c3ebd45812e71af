"""ctypes binding of ``libnvrx_straggler_hip.so`` (C ABI: ``include/nvrx_straggler.h``).

There is deliberately no fallback here: if the HIP library is missing or cannot be loaded the
import of the product path fails with a clear error.  ``torch`` is imported first so that the
library resolves ``libamdhip64.so.7`` to the HIP runtime PyTorch-ROCm already loaded (one runtime
per process: device pointers and streams are shared with torch).
"""
from __future__ import annotations

import ctypes
import os
import threading
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_size_t, c_uint32, c_uint64, c_void_p

_LIB_NAME = "libnvrx_straggler_hip.so"
# NVRX_DEBUG_LIB_DIR: load the native libraries from another directory (the sanitizer build of `make -C csrc asan` lives in
# lib_asan/; tools/run_sanitized.sh points here)
_LIB_PATH = os.path.join(os.environ.get("NVRX_DEBUG_LIB_DIR") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib"), _LIB_NAME)

NVRX_ABI_VERSION = 2
STATS_STRIDE = 8
STAT_MIN, STAT_MAX, STAT_MED, STAT_AVG, STAT_STD, STAT_NUM, STAT_WEIGHT = range(7)
KIND_SECTION, KIND_KERNEL = 0, 1
MAX_RING_CAP = 65536
META_WORDS = 8
ERR_TIMEOUT = -62
ERR_RANGE = -34
ERR_INVALID = -22
ERR_STATE = -1
ATTR_MAX_TOP = 16  # NVRX_ATTR_MAX_TOP
TAIL_Q_PPM_MIN, TAIL_Q_PPM_MAX = 500000, 999999  # the accepted range of a tail quantile, in parts per million
ROUTE_SINGLE, ROUTE_ROWS, ROUTE_ROWS_PRE, ROUTE_TILE16, ROUTE_TILE8 = 1, 2, 3, 4, 5  # NVRX_SCORE_ROUTE_*: what nvrx_score_route returns
ROBUST_MAX_RANKS = 65536  # NVRX_ROBUST_MAX_RANKS
PEER_MAX_GROUPS = 4096  # NVRX_PEER_MAX_GROUPS
ONSET_SEG_PPM_MIN, ONSET_SEG_PPM_MAX = 1, 500000  # the accepted range of an onset's minimum segment, in parts per million
ONSET_MIN_SEG_SAMPLES = 8  # ... and the segment's floor in samples
ONSET_PLANES = 6  # NVRX_ONSET_PLANES: {e, before, after, strength, ago, n} per kernel id and section id
PERIOD_MAX = 4096  # NVRX_PERIOD_MAX: the largest max_period
PERIOD_MIN_CYCLES = 4  # NVRX_PERIOD_MIN_CYCLES: a period repeats at least that often within its row
PERIOD_PLANES = 7  # NVRX_PERIOD_PLANES: {e, peak, rest, strength, period, ago, n} per kernel id and section id
EPISODE_LEN_PPM_MIN, EPISODE_LEN_PPM_MAX = 1, 333333  # the accepted range of an episode's minimum length, in parts per million
EPISODE_MIN_SAMPLES = 8  # ... and the length's floor in samples
EPISODE_PLANES = 7  # NVRX_EPISODE_PLANES: {e, inside, outside, strength, length, ago, n} per kernel id and section id
HISTORY_MAX_DEPTH = 64  # NVRX_HISTORY_MAX_DEPTH: the largest depth H of a score history (the smallest is 2)
HISTORY_RECORD_WORDS = 8  # {latest, median, worst, best, streak, below, present, depth} per (rank, family, slot)
TREND_RECORD_WORDS = 4  # {f32 slope, f32 level, i32 S, u32 usable} per (rank, family, slot)
SLACK_COLS = 64  # NVRX_SLACK_COLS: columns the collective keys are folded into (digest % 64)
SLACK_HEAD_WORDS = 8 + 4 * SLACK_COLS  # the job record and the column records in front of the rank records
SLACK_RANK_WORDS = 8  # {f32 collective_us, waited_us, compute_us, share, u32 calls, columns, 0, 0} per rank
SLACK_GROUP_HEAD_WORDS = 8 + 4 * SLACK_COLS  # per group of nvrx_slack_group_score: its record and its 64 pair records
WORK_MAX_RANKS = 4096  # NVRX_WORK_MAX_RANKS: the most ranks a work-group step compares pairwise
WORK_RANK_WORDS = 8  # {i32 root, u32 size, degree, i32 nearest, u32 nearest_unlike, nearest_either, kernels, sections} per rank
WORK_JOB_WORDS = 4  # {u32 groups, singletons, largest, ranks_with_data}



class ReportDesc(ctypes.Structure):
    """``nvrx_report_desc`` (include/nvrx_straggler.h): one report's buffers and switches, filled once per shape."""

    _fields_ = [
        ("R", c_int32), ("K", c_int32), ("S", c_int32), ("names_ok", c_int32), ("rows_active", c_int32),
        ("do_indiv", c_int32), ("do_rel", c_int32), ("stats_rows", c_int32),
        ("thresholds", c_double * 4),
        ("d_stats", c_void_p), ("d_send", c_void_p), ("d_table", c_void_p),
        ("d_scores", c_void_p), ("d_flags", c_void_p), ("d_meta", c_void_p), ("d_stats_dst", c_void_p),
        ("d_done_counter", c_void_p),
        ("allgather_fn", c_void_p), ("comm", c_void_p), ("send_count", c_int32), ("seq", c_uint32),
        ("h_seq_word", c_void_p), ("timeout_s", c_double),
        ("order_after_stream", c_void_p), ("order_after_enabled", c_int32), ("resident", c_int32), ("prev_settled", c_int32), ("guard_rings", c_int32),
    ]


class WindowDesc(ctypes.Structure):
    """``nvrx_window_desc`` (include/nvrx_straggler.h): what ``nvrx_window_report`` does around the report itself."""

    _fields_ = [
        ("kt_sync", c_void_p), ("kt_hold", c_void_p), ("kt_counter", c_void_p), ("kt_patience_s", c_double),
        ("kt_rows_known", ctypes.c_uint64), ("kt_keys_without_row", ctypes.c_uint64),
        ("rows_used", c_int32), ("asynchronous", c_int32), ("harvest_regions", c_int32), ("out_names_ok", c_int32),
    ]


WINDOW_MISS, WINDOW_NAMES = 1, 2

# every symbol include/nvrx_straggler.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("nvrx_abi_version", c_int, []),
    ("nvrx_last_error", c_char_p, []),
    ("nvrx_row_stats", c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    ("nvrx_score", c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, POINTER(c_double), c_void_p, c_void_p, c_void_p,
                           c_void_p, c_uint32, c_void_p, c_void_p, c_int, c_void_p]),
    ("nvrx_score_route", c_int, [c_int, c_int, c_int, c_void_p, c_void_p]),
    ("nvrx_attribute", c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    ("nvrx_row_quantile", c_int, [c_void_p, c_void_p, c_int, c_int, c_uint32, c_void_p, c_void_p]),
    ("nvrx_tail_score", c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    ("nvrx_row_onset", c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_uint32, c_void_p, c_void_p]),
    ("nvrx_onset_score", c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    ("nvrx_row_period", c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    ("nvrx_period_score", c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    ("nvrx_row_episode", c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_uint32, c_void_p, c_void_p]),
    ("nvrx_episode_score", c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    ("nvrx_robust_score", c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p]),
    ("nvrx_peer_score", c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    ("nvrx_pace_score", c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    ("nvrx_pace_group_score", c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                      c_void_p]),
    ("nvrx_node_score", c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                c_void_p]),
    ("nvrx_score_history", c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_uint64, POINTER(c_double),
                                   c_void_p, c_void_p]),
    ("nvrx_score_trend", c_int, [c_void_p, c_int, c_int, c_int, c_int, c_uint64, c_void_p, c_void_p]),
    ("nvrx_peer_history", c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_uint64, POINTER(c_double), c_void_p,
                                  c_void_p]),
    ("nvrx_peer_trend", c_int, [c_void_p, c_int, c_int, c_int, c_int, c_uint64, c_void_p, c_void_p]),
    ("nvrx_slack_score", c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    ("nvrx_slack_group_score", c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p,
                                       c_void_p]),
    ("nvrx_rowfam_group_score", c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int,
                                        c_void_p, c_void_p]),
    ("nvrx_work_words", c_int, [c_int, c_int, c_int]),
    ("nvrx_work_groups", c_int, [c_void_p, c_int, c_int, c_int, c_float, c_int, c_void_p, c_void_p]),
    ("nvrx_ctx_create", c_int, [c_int, c_int, c_int, c_int, POINTER(c_void_p)]),
    ("nvrx_ctx_destroy", c_int, [c_void_p]),
    ("nvrx_ctx_set_stream", c_int, [c_void_p, c_void_p]),
    ("nvrx_ctx_info", c_int, [c_void_p, c_int]),
    ("nvrx_row_alloc", c_int, [c_void_p, c_int]),
    ("nvrx_row_configure", c_int, [c_void_p, c_int, c_int, c_int]),
    ("nvrx_ring_push", c_int, [c_void_p, c_int, c_float]),
    ("nvrx_ring_push_many", c_int, [c_void_p, c_int, c_void_p, c_int]),
    ("nvrx_ring_push_pairs", c_int, [c_void_p, c_void_p, c_void_p, c_int]),
    ("nvrx_ring_push_staged", c_int, [c_void_p, c_void_p, c_void_p, c_int]),
    ("nvrx_sink_push", c_int, [c_void_p, c_void_p, c_void_p, c_int]),
    ("nvrx_sink_row_alloc", c_int, [c_void_p, c_int]),
    ("nvrx_ring_push_device", c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p]),
    ("nvrx_ring_push_device_rows", c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_void_p]),
    ("nvrx_ring_set_count", c_int, [c_void_p, c_int, c_int]),
    ("nvrx_ring_set_count_all", c_int, [c_void_p, c_int]),
    ("nvrx_ring_count", c_int, [c_void_p, c_int]),
    ("nvrx_ring_counts", c_int, [c_void_p, c_void_p, c_int]),
    ("nvrx_ring_occupancy_changed", c_int, [c_void_p, c_int]),
    ("nvrx_window_report", c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    ("nvrx_window_clocks", c_int, [POINTER(c_double)]),
    ("nvrx_ring_reset", c_int, [c_void_p]),
    ("nvrx_history_reset", c_int, [c_void_p, c_void_p]),
    ("nvrx_ring_flush", c_int, [c_void_p, c_void_p]),
    ("nvrx_ring_read", c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p]),
    ("nvrx_event_begin", c_int, [c_void_p, c_int, c_void_p]),
    ("nvrx_event_end", c_int, [c_void_p, c_int, c_void_p]),
    ("nvrx_event_harvest", c_int, [c_void_p, c_int]),
    ("nvrx_stamp_begin", c_int, [c_void_p, c_int, c_void_p]),
    ("nvrx_stamp_end", c_int, [c_void_p, c_int, c_int, c_float, c_void_p]),
    ("nvrx_report_local", c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    ("nvrx_report", c_int, [c_void_p, POINTER(ReportDesc), c_void_p]),
    ("nvrx_report_issue", c_int, [c_void_p, POINTER(ReportDesc), c_void_p]),
    ("nvrx_report_wait", c_int, [c_void_p, POINTER(ReportDesc)]),
    ("nvrx_report_attribute", c_int, [c_void_p, POINTER(ReportDesc), c_int, c_int, c_int, c_void_p]),
    ("nvrx_tail_local", c_int, [c_void_p, POINTER(ReportDesc), c_uint32, c_void_p, c_int, c_int, c_int, c_void_p]),
    ("nvrx_onset_enable", c_int, [c_void_p, c_int]),
    ("nvrx_onset_local", c_int, [c_void_p, POINTER(ReportDesc), c_uint32, c_float, c_void_p, c_int, c_int, c_int, c_void_p]),
    ("nvrx_period_local", c_int, [c_void_p, POINTER(ReportDesc), c_int, c_float, c_void_p, c_int, c_int, c_int, c_void_p]),
    ("nvrx_episode_local", c_int, [c_void_p, POINTER(ReportDesc), c_uint32, c_float, c_void_p, c_int, c_int, c_int, c_void_p]),
    ("nvrx_report_robust", c_int, [c_void_p, POINTER(ReportDesc), c_int, c_int, c_int, c_float, c_void_p]),
    ("nvrx_report_peer", c_int, [c_void_p, POINTER(ReportDesc), c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    ("nvrx_report_pace", c_int, [c_void_p, POINTER(ReportDesc), c_int, c_int, c_int, c_void_p]),
    ("nvrx_report_pace_group", c_int, [c_void_p, POINTER(ReportDesc), c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                       c_void_p]),
    ("nvrx_report_node", c_int, [c_void_p, POINTER(ReportDesc), c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    ("nvrx_report_history", c_int, [c_void_p, POINTER(ReportDesc), c_int, c_int, c_void_p, c_int, c_int, c_uint64,
                                    POINTER(c_double), c_void_p]),
    ("nvrx_report_trend", c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_uint64, c_void_p]),
    ("nvrx_report_peer_history", c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_uint64, POINTER(c_double),
                                         c_void_p]),
    ("nvrx_report_peer_trend", c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_uint64, c_void_p]),
    ("nvrx_report_work", c_int, [c_void_p, POINTER(ReportDesc), c_float, c_int, c_void_p]),
    ("nvrx_slack_local", c_int, [c_void_p, POINTER(ReportDesc), c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p]),
    ("nvrx_report_clocks", c_int, [POINTER(c_double)]),
    ("nvrx_report_desc_size", c_int, []),
    ("nvrx_peer_create", c_int, [c_int, c_int, c_int, c_int, POINTER(c_void_p)]),
    ("nvrx_peer_ipc_handle", c_int, [c_void_p, c_void_p]),
    ("nvrx_peer_connect", c_int, [c_void_p, c_int, c_void_p]),
    ("nvrx_peer_device_id", c_int, [c_void_p, c_char_p, c_int]),
    ("nvrx_peer_check_access", c_int, [c_void_p, c_int, c_char_p]),
    ("nvrx_peer_ready", c_int, [c_void_p, c_double]),
    ("nvrx_peer_allgather", c_int, [c_void_p, c_void_p, c_size_t, c_int, c_void_p, c_void_p]),
    ("nvrx_peer_allgather_address", c_void_p, []),
    ("nvrx_peer_error", c_int, [c_void_p, POINTER(c_uint32)]),
    ("nvrx_peer_destroy", c_int, [c_void_p]),
    ("nvrx_send_init", c_int, [c_void_p, c_int, c_int, c_int, c_void_p]),
    ("nvrx_timing_enable", c_int, [c_void_p, c_int]),
    ("nvrx_timing_read", c_int, [c_void_p, POINTER(c_double), POINTER(c_int), c_int]),
    ("nvrx_host_alloc", c_int, [POINTER(c_void_p), POINTER(c_void_p), c_size_t]),
    ("nvrx_poll_u32", c_int, [c_void_p, c_uint32, c_double]),
    ("nvrx_host_free", c_int, [c_void_p]),
    ("nvrx_device_alloc", c_int, [c_void_p, c_size_t]),
    ("nvrx_device_free", c_int, [c_void_p]),
    ("nvrx_d2h_sync", c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    ("nvrx_copy_to_host", c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    ("nvrx_wait", c_int, [c_void_p]),
]

# entry points that return a size, not a code (bound like SYMBOLS)
SIZE_SYMBOLS = [
    ("nvrx_rowfam_group_words", c_size_t, [c_int, c_int, c_int, c_int]),
]

_lib = None
_lock = threading.Lock()


class NativeError(RuntimeError):
    """A call into libnvrx_straggler_hip.so failed (message from nvrx_last_error())."""


def lib_path() -> str:
    return _LIB_PATH


def load() -> ctypes.CDLL:
    """Load the HIP library (once).  Raises RuntimeError if it is missing -- never falls back."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(_LIB_PATH):
            raise RuntimeError(
                f"{_LIB_NAME} not found at {_LIB_PATH}. Build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C nvidia-resiliency-ext_amd/csrc`. "
                "The MI355X straggler path has no CPU fallback."
            )
        import torch  # noqa: F401  (load PyTorch-ROCm's HIP runtime first; see module docstring)

        try:
            lib = ctypes.CDLL(_LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        except OSError as e:  # pragma: no cover
            raise RuntimeError(f"failed to load {_LIB_PATH}: {e}") from e
        for name, restype, argtypes in SYMBOLS + SIZE_SYMBOLS:
            fn = getattr(lib, name)  # AttributeError if the library does not export the symbol
            fn.restype = restype
            fn.argtypes = argtypes
        if lib.nvrx_abi_version() != NVRX_ABI_VERSION:
            raise RuntimeError(f"{_LIB_NAME} ABI {lib.nvrx_abi_version()} != expected {NVRX_ABI_VERSION}")
        if lib.nvrx_report_desc_size() != ctypes.sizeof(ReportDesc):
            raise RuntimeError(f"nvrx_report_desc is {lib.nvrx_report_desc_size()} bytes in {_LIB_NAME}, "
                               f"{ctypes.sizeof(ReportDesc)} in the ctypes binding")
        _lib = lib
    return _lib


def check(rc: int) -> int:
    """Turn a negative return code into NativeError carrying the library's message."""
    if rc < 0:
        msg = load().nvrx_last_error()
        raise NativeError(f"nvrx error {rc}: {msg.decode() if msg else '?'}")
    return rc


def table_len(K: int, S: int) -> int:
    return 2 * (K + S) + K + 1


def score_len(S: int) -> int:
    return 2 + 2 * S


def attr_words(n_ranks: int, top_n: int) -> int:
    """NVRX_ATTR_WORDS: 32-bit words of an attribution block ``[n_ranks][2][1 + top_n][4]``."""
    return n_ranks * 2 * (1 + top_n) * 4


def robust_words(n_ranks: int, K: int, S: int) -> int:
    """NVRX_ROBUST_WORDS: 32-bit words of a robust-score block: ``[K+S][4]`` column records, then ``[n_ranks][2][1 + S]``."""
    return 4 * (K + S) + n_ranks * 2 * (1 + S)


def peer_words(G: int, n_ranks: int, K: int, S: int) -> int:
    """NVRX_PEER_WORDS: 32-bit words of a peer-score block: ``[G][K+S][4]`` column records, then ``[n_ranks][1 + S]``."""
    return 4 * G * (K + S) + n_ranks * (1 + S)


def pace_words(n_ranks: int, K: int, S: int) -> int:
    """NVRX_PACE_WORDS: 32-bit words of a pace-score block: ``[K+S][4]`` column records, then ``[n_ranks][2][8]``."""
    return 4 * (K + S) + 16 * n_ranks


def pace_group_words(G: int, n_ranks: int, K: int, S: int) -> int:
    """NVRX_PACE_GROUP_WORDS: 32-bit words of a block of pace scores per peer group: ``[G][K+S][4]`` column records, then
    ``[n_ranks][2][8]``."""
    return 4 * G * (K + S) + 16 * n_ranks


def node_words(G: int, n_ranks: int, K: int, S: int) -> int:
    """NVRX_NODE_WORDS: 32-bit words of a node-score block: ``[G][K+S][4]`` pair records, ``[K+S][4]`` column records across
    the nodes, ``[G][2][8]`` node records, then ``[n_ranks][2][8]`` rank records."""
    return 4 * G * (K + S) + 4 * (K + S) + 16 * G + 16 * n_ranks


def history_stride(H: int) -> int:
    """NVRX_HISTORY_STRIDE: ring positions a history cell of depth ``H`` occupies: 16, 32 or 64, the smallest that is >= H."""
    return 16 if H <= 16 else 32 if H <= 32 else 64


def history_floats(n_ranks: int, S_cap: int, H: int) -> int:
    """NVRX_HISTORY_FLOATS: floats of a history ring ``[n_ranks][2][1 + S_cap][stride]``."""
    return n_ranks * 2 * (1 + S_cap) * history_stride(H)


def history_words(n_ranks: int, S: int) -> int:
    """NVRX_HISTORY_WORDS: 32-bit words of a history step's records ``[n_ranks][2][1 + S][8]``."""
    return n_ranks * 2 * (1 + S) * HISTORY_RECORD_WORDS


def trend_words(n_ranks: int, S: int) -> int:
    """NVRX_TREND_WORDS: 32-bit words of a trend step's records ``[n_ranks][2][1 + S][4]``."""
    return n_ranks * 2 * (1 + S) * TREND_RECORD_WORDS


def peer_history_floats(n_ranks: int, S_cap: int, H: int) -> int:
    """NVRX_PEER_HISTORY_FLOATS: floats of a peer-score history ring ``[n_ranks][1 + S_cap][stride]``."""
    return n_ranks * (1 + S_cap) * history_stride(H)


def peer_history_words(n_ranks: int, S: int) -> int:
    """NVRX_PEER_HISTORY_WORDS: 32-bit words of a peer-history step's records ``[n_ranks][1 + S][8]``."""
    return n_ranks * (1 + S) * HISTORY_RECORD_WORDS


def peer_trend_words(n_ranks: int, S: int) -> int:
    """NVRX_PEER_TREND_WORDS: 32-bit words of a peer-trend step's records ``[n_ranks][1 + S][4]``."""
    return n_ranks * (1 + S) * TREND_RECORD_WORDS


def slack_words(R: int) -> int:
    """NVRX_SLACK_WORDS: 32-bit words of a slack score's output -- job record | 64 column records | ``R`` rank records."""
    return SLACK_HEAD_WORDS + SLACK_RANK_WORDS * R


def slack_group_words(G: int, R: int) -> int:
    """NVRX_SLACK_GROUP_WORDS: 32-bit words of the slack scores per peer group -- ``G`` group records | ``G x 64`` pair records
    | ``R`` rank records."""
    return 8 * G + 256 * G + 8 * R


def rowfam_group_words(G: int, K: int, S: int, n_ranks: int) -> int:
    """NVRX_ROWFAM_GROUP_WORDS: 32-bit words of a row family's scores per peer group -- ``[G][K+S][4]`` column records, then
    ``[n_ranks][1 + S]``."""
    return 4 * G * (K + S) + n_ranks * (1 + S)


def work_offsets(R: int, K: int, S: int):
    """Where the parts of a work-group block start, in 32-bit words -- ``(adjacency, partial nearest, rank records, job record,
    size)``; the signature plane starts at 0 and every part on a 16-byte boundary.  The size is ``nvrx_work_words(R, K, S)``."""
    T = -(-R // 64)
    adj = (R * (K + S) + 3) & ~3
    part = adj + ((2 * R * T + 3) & ~3)
    rank = part + 4 * R * T
    job = rank + WORK_RANK_WORDS * R
    return adj, part, rank, job, job + WORK_JOB_WORDS


def work_words(R: int, K: int, S: int) -> int:
    """``nvrx_work_words``: 32-bit words of a work-group block -- signatures | adjacency | partial nearest | ``R`` rank records |
    job record."""
    return work_offsets(R, K, S)[4]


def tail_q_ppm(q) -> int:
    """A tail quantile as the library carries it: ``round(q * 1e6)``; 0 / None = off, else within [0.5, 0.999999].
    ``ValueError`` for anything else."""
    if q is None:
        return 0
    try:
        ppm = int(round(float(q) * 1e6))
    except (TypeError, ValueError):
        raise ValueError(f"tail_quantile must be a number: 0 (off) or within [0.5, 0.999999], got {q!r}") from None
    if ppm != 0 and not TAIL_Q_PPM_MIN <= ppm <= TAIL_Q_PPM_MAX:
        raise ValueError(f"tail_quantile must be 0 (off) or within [0.5, 0.999999], got {q!r}")
    return ppm


def tail_rank(q_ppm: int, n: int) -> int:
    """Index, in the row sorted ascending, of the nearest-rank ``q_ppm / 1e6`` quantile of ``n >= 1`` samples:
    ``ceil(q * n) - 1`` in integers, exactly as k_row_quantile computes it."""
    return (q_ppm * n + 999999) // 1000000 - 1


def onset_seg_ppm(frac) -> int:
    """An onset's minimum segment as the library carries it: ``round(frac * 1e6)``, within [0.000001, 0.5].  ``ValueError``
    for anything else."""
    try:
        ppm = int(round(float(frac) * 1e6))
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"onset_min_segment must be a number within [0.000001, 0.5], got {frac!r}") from None
    if not ONSET_SEG_PPM_MIN <= ppm <= ONSET_SEG_PPM_MAX:
        raise ValueError(f"onset_min_segment must be within [0.000001, 0.5], got {frac!r}")
    return ppm


def onset_min_segment(seg_ppm: int, n: int) -> int:
    """Samples either side of an onset in a row of ``n``: ``max(8, ceil(seg_ppm * n / 1e6))`` in integers, exactly as
    k_row_onset computes it.  A row shorter than twice that has no onset."""
    return max(ONSET_MIN_SEG_SAMPLES, (seg_ppm * n + 999999) // 1000000)


def period_max(value) -> int:
    """A report's largest candidate period as the library carries it: an integer within [2, 4096].  ``ValueError`` for
    anything else."""
    try:
        p = int(value)
        if p != value:
            raise ValueError
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"period_max must be an integer within [2, {PERIOD_MAX}], got {value!r}") from None
    if not 2 <= p <= PERIOD_MAX:
        raise ValueError(f"period_max must be within [2, {PERIOD_MAX}], got {value!r}")
    return p


def episode_len_ppm(frac) -> int:
    """An episode's minimum length as the library carries it: ``round(frac * 1e6)``, within [0.000001, 0.333333] (an
    episode needs that many samples of "normal" either side as well: three of them fill the row).  ``ValueError`` for
    anything else."""
    try:
        ppm = int(round(float(frac) * 1e6))
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"episode_min_length must be a number within [0.000001, 0.333333], got {frac!r}") from None
    if not EPISODE_LEN_PPM_MIN <= ppm <= EPISODE_LEN_PPM_MAX:
        raise ValueError(f"episode_min_length must be within [0.000001, 0.333333], got {frac!r}")
    return ppm


def episode_min_samples(len_ppm: int, n: int) -> int:
    """Samples of an episode, and of the stretches either side of it, in a row of ``n``: ``max(8, ceil(len_ppm * n / 1e6))``
    in integers, exactly as k_row_episode computes it.  A row shorter than three times that has no episode."""
    return max(EPISODE_MIN_SAMPLES, (len_ppm * n + 999999) // 1000000)
