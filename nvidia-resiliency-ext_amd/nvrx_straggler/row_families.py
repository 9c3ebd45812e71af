"""The row families: score families computed from the ring rows of a report's window -- tail, onset, period, episode.

All four are ONE pipeline with a different ring kernel in front ("Row families")::

    ring kernel by gid into [local_ranks][P][K+S] behind a -1 fill -> [all-gather] -> score kernel on plane 0 with pitch
    P * (K+S) -> one buffer, one ordered D2H on first read -> per-rank records + gpu_relative / section_relative

``FAMILIES`` says what differs, once, in the fixed order the families run in (and issue their collectives in).  The backend
(``Workspace.family_buffers``, ``HipBackend._family_score``, ``HipRings._family_local``) and the reports
(``reporting._RowFamilySource``, ``ReportGenerator._ring_steps``) are written against these records; a further family is
a kernel file, one record here, its two public ``Report`` methods and the one-line delegations by name on the backend, the
workspace and the rings.
"""
from __future__ import annotations

import dataclasses
from typing import Any, Callable, Tuple

from . import _native


def _tail_record(v, params):
    t, = v
    return None if t == -1.0 else t  # (-1: the rank has no samples in this row)


def _onset_record(v, params):
    e, before, after, strength, ago, n = v
    if e == -1.0:  # (-1: the rank has no samples in this row)
        return None
    return {"shift": e, "before": before, "after": after, "strength": strength, "samples_ago": int(ago), "window": int(n)}


def _period_record(v, params):
    e, peak, rest, strength, period, ago, n = v
    if e == -1.0:  # (-1: the rank has no samples in this row)
        return None
    return {"period": int(period), "samples_ago": int(ago), "peak": peak, "rest": rest, "excess": e, "strength": strength,
            "window": int(n)}


def _episode_record(v, params):
    e, inside, outside, strength, length, ago, n = v
    if e == -1.0:  # (-1: the rank has no samples in this row)
        return None
    length, ago, n = int(length), int(ago), int(n)
    return {"length": length, "samples_ago": ago, "began_ago": ago + length if length else 0, "window": n,
            "inside": inside, "outside": outside, "strength": strength, "excess": e,
            "open_ended": bool(length) and ago == _native.episode_min_samples(params[0], n)}


@dataclasses.dataclass(frozen=True)
class RowFamily:
    name: str                 # "tail": Report.tail_scores / identify_tail_stragglers, rings.tail_local, backend.tail_score
    planes: int               # P; a family of one plane has a table [R][K+S], not [R][1][K+S]
    c_row: str                # the three C entry points: the stateless row operator,
    c_score: str              # ... the score kernel on the gathered table
    c_local: str              # ... and the ring kernel of a report's window
    option: str               # the ReportGenerator option that switches the family on
    param_attrs: Tuple[str, ...]  # the generator attributes that hold its parameters; the first is 0 while it is off
    needs_starts: bool        # whether its ring kernel walks the window in time order (rings.onset_enable's snapshot)
    slot: str                 # where a Report keeps it in its __dict__
    stem: str                 # "tails": the report's section_tails / kernel_tails, the backend's tails_copy_out
    record: Callable[[Any, tuple], Any]  # the P planes of one column of one rank -> its record; None: no samples
    footer: Callable[[tuple], dict]      # the parameters as the report's dict states them
    footer_first: bool = False
    score_params: int = 0     # how many of its parameters backend.<name>_score is given as well
    aliases: Tuple[Tuple[str, str], ...] = ()  # further names of a report's mappings: (alias, key)

    def params(self, generator) -> tuple:
        """The family's parameters as ``generator`` holds them; ``()`` while the family is off."""
        if not getattr(generator, self.param_attrs[0]):
            return ()
        return tuple(getattr(generator, a) for a in self.param_attrs)

    def label(self, params: tuple) -> str:
        """The option as error messages name it."""
        return f"{self.option}={params[0] / 1e6}" if self.name == "tail" else self.option


FAMILIES: Tuple[RowFamily, ...] = (
    RowFamily("tail", 1, "nvrx_row_quantile", "nvrx_tail_score", "nvrx_tail_local", "tail_quantile",
              ("tail_q_ppm",), False, "_tail", "tails", _tail_record,
              lambda p: {"quantile": p[0] / 1e6}, footer_first=True, score_params=1),
    RowFamily("onset", _native.ONSET_PLANES, "nvrx_row_onset", "nvrx_onset_score", "nvrx_onset_local", "onset_detection",
              ("onset_seg_ppm", "onset_min_strength"), True, "_onset", "onsets", _onset_record,
              lambda p: {"min_segment": p[0] / 1e6, "min_strength": p[1]}),
    RowFamily("period", _native.PERIOD_PLANES, "nvrx_row_period", "nvrx_period_score", "nvrx_period_local", "period_detection",
              ("period_max", "period_min_strength"), True, "_period", "periods", _period_record,
              lambda p: {"max_period": p[0], "min_strength": p[1]}),
    RowFamily("episode", _native.EPISODE_PLANES, "nvrx_row_episode", "nvrx_episode_score", "nvrx_episode_local",
              "episode_detection", ("episode_len_ppm", "episode_min_strength"), True, "_episode", "episodes", _episode_record,
              lambda p: {"min_length": p[0] / 1e6, "min_strength": p[1]},
              aliases=(("section_scores", "section_relative"), ("gpu_scores", "gpu_relative"))),
)
BY_NAME = {f.name: f for f in FAMILIES}
TAIL, ONSET, PERIOD, EPISODE = FAMILIES
