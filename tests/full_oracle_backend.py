"""The composed CPU checker backend: every follow-up result a report can carry, in ONE backend -- TEST INFRASTRUCTURE, lives
outside the product.

``RowGroupOracleBackend`` and ``SlackGroupOracleBackend`` are siblings under ``PeerHistoryOracleBackend``: the first lacks
``slack_group_score``, the second the four ``*_group_score`` methods, so neither serves a report with both ``row_peer_groups``
and ``slack_peer_groups``.  Both have a cooperative ``__init__(*a, **kw)``, and the method resolution order of
``FullOracleBackend`` puts both on top of the whole chain (attribution, robust, tail ... episode, history, trend, slack, peer,
pace, pace-group, node, work, peer history) with the call counters of either.  It adds nothing of its own: a feature that
lands later extends the chain (or this class' bases) and tests/full_report_script.py's ``FEATURES``, not another sibling.
"""
from row_group_oracle_backend import RowGroupOracleBackend
from slack_group_oracle_backend import SlackGroupOracleBackend


class FullOracleBackend(RowGroupOracleBackend, SlackGroupOracleBackend):
    """The CPU checker with everything a report can carry: the row families per peer group AND the slack scores per peer
    group on top of the peer-score history and everything below it (all computed at enqueue time)."""

    name = "oracle-test+full"
