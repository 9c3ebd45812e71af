"""The report options' rules, once: what ``ReportGenerator.__init__`` checks, how ``Detector.initialize`` reads a default from
the environment, and which keywords ``Detector`` and ``FoldedJob`` hand on together ("Report options").

Plain functions that return the checked value or raise the constructor's own message; the message's wording belongs to the
option, so every function takes it as text and normalises nothing.  ``GROUPS`` says, as data, which keywords travel together
and what switches them on.  Internal: ``reporting``, ``straggler`` and ``folded`` import it, nobody else.
"""
from __future__ import annotations

import dataclasses
import os
from typing import Any, Callable, Mapping, Optional, Sequence, Tuple

import numpy as np

from . import _native
from . import backend as _backend_mod


# ---- value checks ------------------------------------------------------------------------------------------------------------
def integer(name: str, value, text: str, lo: int, hi: Optional[int] = None, zero_is_off: bool = False) -> int:
    """``value`` as an ``int``: an integer, not a bool, within [``lo``, ``hi``] (or 0 where that means off); else
    "``name`` must be ``text``, got ..."."""
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not (
            (lo <= value and (hi is None or value <= hi)) or (zero_is_off and value == 0)):
        raise ValueError(f"{name} must be {text}, got {value!r}")
    return int(value)


def floats(values: Sequence, message: str) -> list:
    """``float()`` of every value, for options whose message names them together; one that is no number raises ``message``."""
    try:
        return [float(v) for v in values]
    except (TypeError, ValueError):
        raise ValueError(message) from None


def within(name: str, value, x: float, text: str, lo: float, hi: float, *, lo_open: bool = False, hi_open: bool = False,
           no_bool: bool = False) -> float:
    """``x``, which is ``float(value)``, where it lies within the range (and ``value`` is no bool, where the option minds);
    else "``name`` must be ``text``, got ..."."""
    inside = (lo < x if lo_open else lo <= x) and (x < hi if hi_open else x <= hi)  # (NaN fails every comparison)
    if not inside or (no_bool and isinstance(value, bool)):
        raise ValueError(f"{name} must be {text}, got {value!r}")
    return x


def number(name: str, value, text: str, lo: float, hi: float, *, no_number_text: Optional[str] = None, **range_options) -> float:
    """``value`` as a ``float`` within the range.  ``no_number_text``: the text for a value that is no number at all, where
    the option words that differently from a number out of range."""
    x, = floats((value,), f"{name} must be {no_number_text or text}, got {value!r}")
    return within(name, value, x, text, lo, hi, **range_options)


def share(name: str, value) -> float:
    """A share of a row's variance (the ``*_min_strength`` options, ``robust_floor``): a number within [0, 1]."""
    return number(name, value, "within [0, 1]", 0.0, 1.0, no_number_text="a number within [0, 1]")


# ---- requirements ------------------------------------------------------------------------------------------------------------
def needs_relative(label: str, scores_to_compute, reason: str) -> None:
    if "relative_perf_scores" not in scores_to_compute:
        raise ValueError(f"{label} needs relative_perf_scores among scores_to_compute (got {scores_to_compute!r}): {reason}")


def needs_backend(label: str, noun: str, *methods: str) -> None:
    """The active backend has every one of ``methods``; else the message names the first it lacks."""
    be = _backend_mod._backend  # (an engine that does not exist yet is the HIP engine, which has it)
    lacks = [m for m in methods if be is not None and not hasattr(be, m)]
    if lacks:
        raise RuntimeError(f"{label}: the active backend ({getattr(be, 'name', type(be).__name__)}) has no {noun} "
                           f"(backend.{lacks[0]})")


def needs_with_peer_groups(option: str, base: str, base_on, peer_groups_on, base_label: Optional[str] = None) -> None:
    """A ``*_peer_groups`` option needs its base option and ``peer_groups``; the message says which of them is not set."""
    missing = [name for name, on in ((base_label or base, base_on), ("peer_groups", peer_groups_on)) if not on]
    if missing:
        raise ValueError(f"{option} needs {base} and peer_groups; {' and '.join(missing)} "
                         f"{'is' if len(missing) == 1 else 'are'} not set")


# ---- histories and trends ----------------------------------------------------------------------------------------------------
def history_depth(name: str, value) -> int:
    return integer(name, value, f"0 (off) or an integer within [2, {_native.HISTORY_MAX_DEPTH}] reports", 2,
                   _native.HISTORY_MAX_DEPTH, zero_is_off=True)


def persistence_rule(history: str, depth: int, min_name: str, min_reports, thr_name: str, thresholds, default: tuple,
                     count: int, thr_text: str) -> tuple:
    """``(min_reports, thresholds)`` of the history option ``history`` of ``depth`` reports: a streak within the history, and
    ``count`` finite thresholds (None: ``default``)."""
    m = integer(min_name, min_reports, f"an integer within [1, {history}={depth}]", 1, depth)
    message = f"{thr_name} must be {thr_text}, got {thresholds!r}"
    thr = default if thresholds is None else tuple(floats(thresholds, message))
    if len(thr) != count or not all(np.isfinite(thr)):
        raise ValueError(message)
    return m, thr


def trend_rule(option: str, history: str, depth: int, min_reports, min_tau, horizon) -> tuple:
    """``(trend_min_reports, trend_min_tau, horizon)`` of the trend option ``option`` behind the history option ``history``
    of ``depth`` reports.  None as the horizon is the history's depth."""
    if depth < 4:
        raise ValueError(f"{option} needs a {history.replace('_', ' ')} of at least 4 reports ({history} within [4, "
                         f"{_native.HISTORY_MAX_DEPTH}]), got {history}={depth!r}")
    m = integer("trend_min_reports", min_reports, f"an integer within [4, {history}={depth}]", 4, depth)
    tau = number("trend_min_tau", min_tau, "a number within (0, 1]", 0.0, 1.0, lo_open=True, no_bool=True)
    hz = integer("trend_horizon", depth if horizon is None else horizon,
                 "None (the history's depth) or an integer >= 0 reports", 0)
    return m, tau, hz


# ---- defaults from the environment (Detector.initialize).  The argument wins: the variable is read, and can only be wrong,
# where the argument is None ----
def env_flag(given, name: str):
    """Lenient: unset, "" and "0" are off, anything else is on."""
    if given is not None:
        return given
    return os.environ.get(name, "0") not in ("", "0")


def env_strict_flag(given, name: str):
    """Strict: "1" is on, unset, "" and "0" are off, anything else is an error."""
    if given is not None:
        return given
    value = os.environ.get(name, "")
    if value not in ("", "0", "1"):
        raise ValueError(f"{name} must be 0 or 1, got {value!r}")
    return value == "1"


def env_number(given, name: str, kind: Callable[[str], Any], default, message: str):
    """``kind(value)`` (``int`` or ``float``); unset or "": ``default``.  ``message`` may quote the text as ``{value!r}``."""
    if given is not None:
        return given
    value = os.environ.get(name, "")
    if not value:
        return default
    try:
        return kind(value)
    except ValueError:
        raise ValueError(message.format(value=value)) from None


def env_numbers(given, name: str, message: str):
    """A tuple of comma-separated numbers; unset or "": None (off).  ``message`` may quote the text as ``{value!r}``."""
    if given is not None:
        return given
    value = os.environ.get(name, "")
    if not value.strip():
        return None
    try:
        return tuple(float(v) for v in value.split(","))
    except ValueError:
        raise ValueError(message.format(value=value)) from None


# ---- what Detector and FoldedJob hand to ReportGenerator ---------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class OptionGroup:
    keywords: Tuple[str, ...]  # they travel together; the first switches the group on
    on: Optional[Callable[[Mapping[str, Any]], Any]] = None  # ... unless this says what does


def _auto(v) -> bool:
    return isinstance(v["peer_groups"], str) and v["peer_groups"] == "auto"


# handed on whatever their values (their defaults are the generator's own)
ALWAYS: Tuple[str, ...] = (
    "asynchronous", "kernel_attribution", "tail_quantile", "robust_scores", "onset_detection", "onset_min_segment",
    "onset_min_strength", "period_detection", "period_max", "period_min_strength", "episode_detection", "episode_min_length",
    "episode_min_strength", "score_history", "persistence_min_reports", "persistence_thresholds", "score_trends",
    "trend_min_reports", "trend_min_tau", "trend_horizon", "collective_slack", "slack_min_ranks", "slack_min_share",
    "slack_max_ratio")
# a group that is off is left out: the generator is built exactly as before the option existed
GROUPS: Tuple[OptionGroup, ...] = (
    OptionGroup(("peer_groups", "peer_min_ranks"), on=lambda v: v["peer_groups"] is not None),
    OptionGroup(("peer_history", "peer_persistence_min_reports", "peer_persistence_thresholds", "peer_trends"),
                on=lambda v: v["peer_history"] or v["peer_trends"]),
    OptionGroup(("work_groups", "work_count_tol", "work_max_unlike"), on=lambda v: v["work_groups"] or _auto(v)),
    OptionGroup(("pace_scores", "pace_min_ranks", "pace_min_columns", "pace_min_effect", "pace_min_breadth")),
    # (the generator says which of the base option and peer_groups a *_peer_groups option misses)
    OptionGroup(("pace_peer_groups",)),
    OptionGroup(("robust_peer_groups",)),
    OptionGroup(("slack_peer_groups",)),
    OptionGroup(("row_peer_groups",)),
    OptionGroup(("node_scores", "node_groups", "node_min_members", "node_min_nodes", "node_min_columns", "node_min_effect",
                 "node_min_breadth", "node_min_agree")),
    OptionGroup(("node_peer_groups",)),
    OptionGroup(("peer_attribution",)),  # (the generator validates it and says what it misses)
    OptionGroup(("ramp_detection", "ramp_min_segment", "ramp_min_strength")),
    OptionGroup(("stall_detection", "stall_min_ratio", "stall_min_z", "stall_min_share")),
    OptionGroup(("tail_profile",)),  # (None and () are off)
    OptionGroup(("timeline_scores", "timeline_buckets", "timeline_min_rows", "timeline_min_effect", "timeline_min_breadth",
                 "timeline_min_buckets")),
    OptionGroup(("comovement_groups", "comovement_min_amplitude", "comovement_min_similarity", "comovement_min_ranks")),
)


def forwarded(values: Mapping[str, Any]) -> dict:
    """The keyword arguments for ``ReportGenerator`` out of the resolved ``values`` (which may hold more than options)."""
    kwargs = {k: values[k] for k in ALWAYS}
    for group in GROUPS:
        if group.on(values) if group.on else values[group.keywords[0]]:
            kwargs.update((k, values[k]) for k in group.keywords)
    return kwargs
