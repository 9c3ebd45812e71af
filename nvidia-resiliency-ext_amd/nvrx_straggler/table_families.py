"""The table families: score families that read a report's gathered ``[R][K+S]`` table and rate ranks against each other --
robust, peer-group, pace, pace-per-peer-group and node scores.

The device kernels differ; the host path is ONE ("Table families")::

    settle the slot's last step -> the slot's records buffer -> nvrx_<name>_score on the caller's table, or
    nvrx_report_<name> behind the report just issued -> one uint32 block, one ordered D2H on first read -> cut into arrays

``FAMILIES`` says what differs, once, in the fixed order the families run in.  The backend (``Workspace.table_buffers`` /
``table_settle``, ``HipBackend._table_score`` / ``table_copy_out``, ``HipRings._table_report``, ``TableScores``) is written
against these records; a further family is a kernel file, one record here, its ``Report`` methods and the one-line
delegations by name on the backend, the workspace and the rings.
"""
from __future__ import annotations

import dataclasses
import math
import operator
from typing import Callable, Tuple

import numpy as np

from . import _native

_U32, _F32 = np.uint32, np.float32
_RANKS = ("first_rank", "n_ranks")


@dataclasses.dataclass(frozen=True)
class TableFamily:
    name: str                # "robust": backend.robust_score / robust_copy_out, rings.report_robust
    c_score: str             # the two C entry points: on a caller's table and stream,
    c_report: str            # ... and behind the context's last report
    slot: str                # the workspace's records buffer it uses (pace and pace_group share one: a report runs one of them)
    words: Callable[..., int]  # _native.<name>_words([G,] n_ranks, K, S): 32-bit words of its block
    groups: str              # "": job-wide; else it takes a PeerGroups -- (d_groups, G) lead its C arguments -- and this is
    #                          what a ValueError calls them ("peer", "node")
    max_size: bool           # whether the largest group's size follows G in the C arguments
    c_args: Tuple[str, ...]  # the rank range and the family's parameters, by name, in C ARGUMENT ORDER
    blocks: Callable[[int, int, int, int], tuple]  # (G, n_ranks, K+S, S) -> ((shape, dtype), ...): its block, in order
    # (worked out from c_args, once: these run at every report)
    params: Tuple[str, ...] = dataclasses.field(init=False)  # the family's parameters, in the order backend.<name>_score and
    #                                                          a TableScores hold them
    _in_c_order: Callable[[tuple], tuple] = dataclasses.field(init=False, repr=False)

    def __post_init__(self):
        params = tuple(a for a in self.c_args if a not in _RANKS)
        object.__setattr__(self, "params", params)
        object.__setattr__(self, "_in_c_order", operator.itemgetter(*((_RANKS + params).index(a) for a in self.c_args)))

    def rank_args(self, first_rank: int, n_ranks: int, params: tuple) -> tuple:
        """The rank range and ``params`` in C argument order."""
        return self._in_c_order((first_rank, n_ranks) + params)

    def n_words(self, G: int, n_ranks: int, K: int, S: int) -> int:
        return self.words(G, n_ranks, K, S) if self.groups else self.words(n_ranks, K, S)

    def cut(self, host: np.ndarray, G: int, n_ranks: int, K: int, S: int) -> tuple:
        """The copied-out uint32 block as the family's arrays (private copies; float fields of uint32 arrays stay bit
        patterns)."""
        out, at = [], 0
        for shape, dtype in self.blocks(G, n_ranks, K + S, S):
            size = math.prod(shape)
            out.append(host[at : at + size].view(dtype).reshape(shape).copy())
            at += size
        return tuple(out)


FAMILIES: Tuple[TableFamily, ...] = (
    # (cols [K+S, 4] uint32 {ctr, mad, scale, n}, scores [n_ranks, 2, 1 + S] f32 {ratio, z})
    TableFamily("robust", "nvrx_robust_score", "nvrx_report_robust", "robust", _native.robust_words, "", False,
                _RANKS + ("min_ranks", "floor_rel"),
                lambda G, n, KS, S: (((KS, 4), _U32), ((n, 2, 1 + S), _F32))),
    # (cols [G, K+S, 4] uint32 {floor, present, floor_rank, members}, scores [n_ranks, 1 + S] f32)
    TableFamily("peer", "nvrx_peer_score", "nvrx_report_peer", "peer", _native.peer_words, "peer", False,
                _RANKS + ("min_ranks",),
                lambda G, n, KS, S: (((G, KS, 4), _U32), ((n, 1 + S), _F32))),
    # (cols [K+S, 4] {ctr, n, above, below}, ranks [n_ranks, 2, 8] {pace, spread, columns, slower, faster, total_us,
    # slower_us, excess_us}) uint32
    TableFamily("pace", "nvrx_pace_score", "nvrx_report_pace", "pace", _native.pace_words, "", False,
                _RANKS + ("min_ranks",),
                lambda G, n, KS, S: (((KS, 4), _U32), ((n, 2, 8), _U32))),
    # (cols [G, K+S, 4], ranks [n_ranks, 2, 8]) uint32: pace's, one set of column records per group
    TableFamily("pace_group", "nvrx_pace_group_score", "nvrx_report_pace_group", "pace", _native.pace_group_words, "peer", True,
                _RANKS + ("min_ranks", "min_peers"),
                lambda G, n, KS, S: (((G, KS, 4), _U32), ((n, 2, 8), _U32))),
    # (pairs [G, K+S, 4] {med, n, above, below}, cols [K+S, 4] {center, nodes, above, below}, nodes [G, 2, 8], ranks
    # [n_ranks, 2, 8]) uint32, the last two spelled as pace's rank records; the thresholds come BEFORE the rank range
    TableFamily("node", "nvrx_node_score", "nvrx_report_node", "node", _native.node_words, "node", True,
                ("min_members", "min_nodes") + _RANKS,
                lambda G, n, KS, S: (((G, KS, 4), _U32), ((KS, 4), _U32), ((G, 2, 8), _U32), ((n, 2, 8), _U32))),
)
BY_NAME = {f.name: f for f in FAMILIES}
ROBUST, PEER, PACE, PACE_GROUP, NODE = FAMILIES
SLOTS: Tuple[TableFamily, ...] = (ROBUST, PEER, PACE, NODE)  # one family per slot, in the order the slots settle
