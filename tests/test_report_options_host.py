"""Report options without a GPU: what the other host tests do not pin.  Which of two bad arguments ``ReportGenerator`` reports
(every block with more than one check), which of two bad ``NVRX_*`` variables ``Detector.initialize`` reports, each with the
WHOLE message; and, per group of options that ``Detector`` and ``FoldedJob`` hand on together, the option attributes the
generator ends up with -- the absent ones included -- with the group on and off.

Every text and dictionary below was recorded from the commit before ``report_options.py`` existed; the file passes there
unchanged."""
import pytest

from full_oracle_backend import FullOracleBackend

IND = ["individual_perf_scores"]
nan = float("nan")


class _Bare:
    """A backend without a single step: every "has no ..." check fails on it."""
    name = "bare"


class _Peers:
    """... and one with the peer step and its history, and no trends."""
    name = "peers"
    peer_score = peer_history = staticmethod(lambda *a, **k: None)


class _Checker(FullOracleBackend):
    """The CPU checker, with the names of the steps it does not restate: construction only asks whether a step exists."""
    robust_group_score = node_group_score = peer_attribute = ramp_score = stall_score = staticmethod(lambda *a, **k: None)


# (the active backend: None, "bare", "full" = the CPU checker as it is, or "peers"; ReportGenerator's keywords, the exception,
# str(exception))
CONSTRUCTOR_CASES = [
    (None, {'robust_scores': True, 'robust_min_ranks': 0, 'robust_floor': 'x'}, ValueError,
     'robust_min_ranks must be an integer >= 1, got 0'),
    (None, {'robust_scores': True, 'robust_floor': 'x', 'scores_to_compute': IND}, ValueError,
     "robust_floor must be a number within [0, 1], got 'x'"),
    (None, {'robust_scores': True, 'robust_floor': 2, 'scores_to_compute': IND}, ValueError,
     'robust_floor must be within [0, 1], got 2'),
    ('bare', {'robust_scores': True, 'scores_to_compute': IND}, ValueError,
     "robust_scores needs relative_perf_scores among scores_to_compute (got ['individual_perf_scores']): robust scores are relative scores"),
    (None, {'peer_groups': 'mod:2', 'peer_min_ranks': 0, 'scores_to_compute': IND}, ValueError,
     'peer_min_ranks must be an integer >= 1, got 0'),
    ('bare', {'peer_groups': 'mod:2', 'scores_to_compute': IND}, ValueError,
     "peer_groups needs relative_perf_scores among scores_to_compute (got ['individual_perf_scores']): peer-group scores are relative scores"),
    (None, {'work_groups': True, 'work_count_tol': 'x', 'work_max_unlike': 2}, ValueError,
     "work_count_tol and work_max_unlike must be numbers, got 'x' and 2"),
    (None, {'work_groups': True, 'work_count_tol': 17, 'work_max_unlike': 2}, ValueError,
     'work_count_tol must be within [0, 16], got 17'),
    (None, {'work_groups': True, 'work_max_unlike': 2, 'scores_to_compute': IND}, ValueError,
     'work_max_unlike must be within [0, 1], got 2'),
    (None, {'peer_groups': 'auto', 'work_count_tol': 17}, ValueError,
     'work_count_tol must be within [0, 16], got 17'),
    ('bare', {'work_groups': True, 'scores_to_compute': IND}, ValueError,
     "work_groups needs relative_perf_scores among scores_to_compute (got ['individual_perf_scores']): work groups compare ranks"),
    (None, {'pace_scores': True, 'pace_min_ranks': 0, 'pace_min_columns': 0}, ValueError,
     'pace_min_ranks must be an integer >= 1, got 0'),
    (None, {'pace_scores': True, 'pace_min_columns': 0, 'pace_min_effect': 'x'}, ValueError,
     'pace_min_columns must be an integer >= 1, got 0'),
    (None, {'pace_scores': True, 'pace_min_effect': 2.0, 'pace_min_breadth': 'x'}, ValueError,
     "pace_min_effect and pace_min_breadth must be numbers, got 2.0 and 'x'"),
    (None, {'pace_scores': True, 'pace_min_effect': 1.0, 'pace_min_breadth': 0}, ValueError,
     'pace_min_effect must be within [0, 1), got 1.0'),
    (None, {'pace_scores': True, 'pace_min_breadth': 0, 'scores_to_compute': IND}, ValueError,
     'pace_min_breadth must be within (0, 1], got 0'),
    ('bare', {'pace_scores': True, 'scores_to_compute': IND}, ValueError,
     "pace_scores needs relative_perf_scores among scores_to_compute (got ['individual_perf_scores']): pace scores are relative scores"),
    (None, {'pace_peer_groups': True}, ValueError,
     'pace_peer_groups needs pace_scores and peer_groups; pace_scores and peer_groups are not set'),
    ('bare', {'pace_peer_groups': True}, ValueError,
     'pace_peer_groups needs pace_scores and peer_groups; pace_scores and peer_groups are not set'),
    (None, {'robust_peer_groups': True}, ValueError,
     'robust_peer_groups needs robust_scores and peer_groups; robust_scores and peer_groups are not set'),
    (None, {'node_peer_groups': True}, ValueError,
     'node_peer_groups needs node_scores and peer_groups; node_scores and peer_groups are not set'),
    (None, {'slack_peer_groups': True}, ValueError,
     'slack_peer_groups needs collective_slack and peer_groups; collective_slack and peer_groups are not set'),
    (None, {'row_peer_groups': True}, ValueError,
     'row_peer_groups needs a row family and peer_groups; a row family (tail_quantile, onset_detection, period_detection, '
     'episode_detection) and peer_groups are not set'),
    (None, {'row_peer_groups': True, 'peer_groups': 'mod:2'}, ValueError,
     'row_peer_groups needs a row family and peer_groups; a row family (tail_quantile, onset_detection, period_detection, '
     'episode_detection) is not set'),
    (None, {'row_peer_groups': True, 'tail_quantile': 0.9}, ValueError,
     'row_peer_groups needs a row family and peer_groups; peer_groups is not set'),
    (None, {'node_scores': True, 'node_min_members': 0, 'node_min_nodes': 0}, ValueError,
     'node_min_members must be an integer >= 1, got 0'),
    (None, {'node_scores': True, 'node_min_nodes': 0, 'node_min_columns': 0}, ValueError,
     'node_min_nodes must be an integer >= 1, got 0'),
    (None, {'node_scores': True, 'node_min_columns': 0, 'node_min_agree': 'x'}, ValueError,
     'node_min_columns must be an integer >= 1, got 0'),
    (None, {'node_scores': True, 'node_min_effect': 1, 'node_min_breadth': 'x'}, ValueError,
     "node_min_effect, node_min_breadth and node_min_agree must be numbers, got 1, 'x' and 0.75"),
    (None, {'node_scores': True, 'node_min_effect': 1, 'node_min_breadth': 0}, ValueError,
     'node_min_effect must be within [0, 1), got 1'),
    (None, {'node_scores': True, 'node_min_breadth': 0, 'node_min_agree': 0}, ValueError,
     'node_min_breadth must be within (0, 1], got 0'),
    (None, {'node_scores': True, 'node_min_agree': 0, 'scores_to_compute': IND}, ValueError,
     'node_min_agree must be within (0, 1], got 0'),
    (None, {'node_scores': True, 'node_groups': 'rack:4', 'scores_to_compute': IND}, ValueError,
     "node_scores needs relative_perf_scores among scores_to_compute (got ['individual_perf_scores']): node scores are relative scores"),
    ('bare', {'node_scores': True, 'node_groups': 'rack:4'}, RuntimeError,
     'node_scores: the active backend (bare) has no node scores (backend.node_score)'),
    (None, {'onset_detection': True, 'onset_min_segment': 0.9, 'onset_min_strength': 'x'}, ValueError,
     'onset_min_segment must be within [0.000001, 0.5], got 0.9'),
    (None, {'onset_detection': True, 'onset_min_strength': 'x', 'scores_to_compute': IND}, ValueError,
     "onset_min_strength must be a number within [0, 1], got 'x'"),
    (None, {'onset_detection': True, 'onset_min_strength': nan, 'scores_to_compute': IND}, ValueError,
     'onset_min_strength must be within [0, 1], got nan'),
    ('bare', {'onset_detection': True, 'scores_to_compute': IND}, ValueError,
     "onset_detection needs relative_perf_scores among scores_to_compute (got ['individual_perf_scores']): onset scores are relative scores"),
    (None, {'period_detection': True, 'period_max': 1, 'period_min_strength': 'x'}, ValueError,
     'period_max must be within [2, 4096], got 1'),
    (None, {'period_detection': True, 'period_min_strength': None, 'scores_to_compute': IND}, ValueError,
     'period_min_strength must be a number within [0, 1], got None'),
    (None, {'period_detection': True, 'period_min_strength': 1.5, 'scores_to_compute': IND}, ValueError,
     'period_min_strength must be within [0, 1], got 1.5'),
    (None, {'episode_detection': True, 'episode_min_length': 0.9, 'episode_min_strength': 'x'}, ValueError,
     'episode_min_length must be within [0.000001, 0.333333], got 0.9'),
    (None, {'episode_detection': True, 'episode_min_strength': 'x', 'scores_to_compute': IND}, ValueError,
     "episode_min_strength must be a number within [0, 1], got 'x'"),
    (None, {'episode_detection': True, 'episode_min_strength': -0.1, 'scores_to_compute': IND}, ValueError,
     'episode_min_strength must be within [0, 1], got -0.1'),
    (None, {'ramp_detection': True, 'ramp_min_segment': 0.9, 'ramp_min_strength': 'x'}, ValueError,
     'ramp_min_segment must be within [0.000001, 0.5], got 0.9'),
    (None, {'ramp_detection': True, 'ramp_min_strength': 'x', 'scores_to_compute': IND}, ValueError,
     "ramp_min_strength must be a number within [0, 1], got 'x'"),
    (None, {'ramp_detection': True, 'ramp_min_strength': 2, 'scores_to_compute': IND}, ValueError,
     'ramp_min_strength must be within [0, 1], got 2'),
    ('bare', {'ramp_detection': True, 'scores_to_compute': IND}, ValueError,
     "ramp_detection needs relative_perf_scores among scores_to_compute (got ['individual_perf_scores']): ramp scores are relative scores"),
    (None, {'stall_detection': True, 'stall_min_ratio': 1.0, 'stall_min_z': 'x'}, ValueError,
     'stall_min_ratio must be within [1.000001, 1000], got 1.0'),
    (None, {'stall_detection': True, 'stall_min_z': 'x', 'stall_min_share': 2}, ValueError,
     "stall_min_z must be a finite number >= 0 and stall_min_share a number within [0, 1), got 'x' and 2"),
    (None, {'stall_detection': True, 'stall_min_z': -1, 'stall_min_share': 2}, ValueError,
     'stall_min_z must be a finite number >= 0, got -1'),
    (None, {'stall_detection': True, 'stall_min_share': 2, 'scores_to_compute': IND}, ValueError,
     'stall_min_share must be within [0, 1), got 2'),
    ('bare', {'stall_detection': True, 'scores_to_compute': IND}, ValueError,
     "stall_detection needs relative_perf_scores among scores_to_compute (got ['individual_perf_scores']): stall scores are relative scores"),
    (None, {'score_history': 8, 'persistence_min_reports': 0, 'persistence_thresholds': (1, 2)}, ValueError,
     'persistence_min_reports must be an integer within [1, score_history=8], got 0'),
    (None, {'score_history': 8, 'persistence_thresholds': 5}, ValueError,
     'persistence_thresholds must be four finite numbers (gpu_rel, section_rel, gpu_indiv, section_indiv), got 5'),
    (None, {'score_history': 8, 'persistence_thresholds': ('a', 1, 1, 1)}, ValueError,
     "persistence_thresholds must be four finite numbers (gpu_rel, section_rel, gpu_indiv, section_indiv), got ('a', 1, 1, 1)"),
    ('bare', {'score_history': 8, 'persistence_thresholds': (1, 2)}, ValueError,
     'persistence_thresholds must be four finite numbers (gpu_rel, section_rel, gpu_indiv, section_indiv), got (1, 2)'),
    (None, {'score_trends': True, 'score_history': 3, 'trend_min_reports': 3}, ValueError,
     'score_trends needs a score history of at least 4 reports (score_history within [4, 64]), got score_history=3'),
    (None, {'score_trends': True, 'score_history': 8, 'trend_min_reports': 3, 'trend_min_tau': 0}, ValueError,
     'trend_min_reports must be an integer within [4, score_history=8], got 3'),
    (None, {'score_trends': True, 'score_history': 8, 'trend_min_tau': 'x', 'trend_horizon': -1}, ValueError,
     "trend_min_tau must be a number within (0, 1], got 'x'"),
    ('bare', {'score_trends': True, 'score_history': 8, 'trend_horizon': -1}, RuntimeError,
     'score_history: the active backend (bare) has no score history (backend.score_history)'),
    (None, {'peer_history': 8, 'peer_persistence_min_reports': 0}, ValueError,
     'peer_history needs peer_groups: it is the history of the peer-group scores'),
    (None, {'peer_history': 8, 'peer_groups': 'mod:2', 'peer_persistence_min_reports': 0, 'peer_persistence_thresholds': (1,)},
     ValueError, 'peer_persistence_min_reports must be an integer within [1, peer_history=8], got 0'),
    (None, {'peer_history': 8, 'peer_groups': 'mod:2', 'peer_persistence_thresholds': 'ab'}, ValueError,
     "peer_persistence_thresholds must be two finite numbers (gpu, section), got 'ab'"),
    (None, {'peer_history': 8, 'peer_groups': 'mod:2', 'peer_persistence_thresholds': (nan, 1)}, ValueError,
     'peer_persistence_thresholds must be two finite numbers (gpu, section), got (nan, 1)'),
    (None, {'peer_trends': True, 'peer_history': 3, 'peer_groups': 'mod:2', 'trend_min_reports': 3}, ValueError,
     'peer_trends needs a peer history of at least 4 reports (peer_history within [4, 64]), got peer_history=3'),
    # (both trends on: the score block accepts 7 of 8 reports, the peer block behind it refuses 7 of 6)
    (None, {'peer_trends': True, 'peer_history': 6, 'peer_groups': 'mod:2', 'score_trends': True, 'score_history': 8,
            'trend_min_reports': 7}, ValueError, 'trend_min_reports must be an integer within [4, peer_history=6], got 7'),
    (None, {'peer_trends': True, 'peer_history': 8, 'peer_groups': 'mod:2', 'trend_min_reports': 3, 'trend_min_tau': 0}, ValueError,
     'trend_min_reports must be an integer within [4, peer_history=8], got 3'),
    (None, {'peer_trends': True, 'peer_history': 8, 'peer_groups': 'mod:2', 'trend_min_tau': 2, 'trend_horizon': -1}, ValueError,
     'trend_min_tau must be a number within (0, 1], got 2'),
    (None, {'peer_trends': True, 'peer_history': 8, 'peer_groups': 'mod:2', 'trend_horizon': 1.5}, ValueError,
     "trend_horizon must be None (the history's depth) or an integer >= 0 reports, got 1.5"),
    (None, {'collective_slack': True, 'slack_min_ranks': 0, 'slack_min_share': -1}, ValueError,
     'slack_min_ranks must be an integer >= 1, got 0'),
    (None, {'collective_slack': True, 'slack_min_share': 'x', 'slack_max_ratio': -1}, ValueError,
     "slack_min_share must be a finite number >= 0, got 'x'"),
    (None, {'collective_slack': True, 'slack_max_ratio': -1, 'scores_to_compute': IND}, ValueError,
     'slack_max_ratio must be a finite number >= 0, got -1'),
    ('bare', {'collective_slack': True, 'scores_to_compute': IND}, ValueError,
     "collective_slack needs relative_perf_scores among scores_to_compute (got ['individual_perf_scores']): slack scores compare ranks"),
    # the "has no ..." messages no other test reaches: a backend with the steps in front of the one that is asked for
    ('full', {'robust_scores': True, 'peer_groups': 'mod:2', 'robust_peer_groups': True}, RuntimeError,
     'robust_peer_groups: the active backend (oracle-test+full) has no robust scores per peer group (backend.robust_group_score)'),
    ('full', {'node_scores': True, 'peer_groups': 'mod:2', 'node_peer_groups': True}, RuntimeError,
     'node_peer_groups: the active backend (oracle-test+full) has no node scores per peer group (backend.node_group_score)'),
    ('full', {'ramp_detection': True}, RuntimeError,
     'ramp_detection: the active backend (oracle-test+full) has no ramp scores (backend.ramp_score)'),
    ('full', {'stall_detection': True}, RuntimeError,
     'stall_detection: the active backend (oracle-test+full) has no stall scores (backend.stall_score)'),
    ('full', {'peer_groups': 'mod:2', 'peer_attribution': 3}, RuntimeError,
     'peer_attribution=3: the active backend (oracle-test+full) has no peer attribution (backend.peer_attribute)'),
    ('peers', {'peer_groups': 'mod:2', 'peer_history': 8, 'peer_trends': True}, RuntimeError,
     'peer_trends: the active backend (peers) has no peer-score trends (backend.peer_trend)'),
]

# (the environment, Detector.initialize's keywords, the exception, str(exception)): the variables are read in a fixed order
DETECTOR_CASES = [
    ({'NVRX_KERNEL_ATTRIBUTION': 'two'}, {}, ValueError,
     'NVRX_KERNEL_ATTRIBUTION must be an integer: 0 (off) or 1..16'),
    ({'NVRX_SCORE_HISTORY': 'x', 'NVRX_PERSISTENCE_MIN_REPORTS': 'y'}, {}, ValueError,
     'NVRX_SCORE_HISTORY must be an integer: 0 (off) or 2..64 reports'),
    ({'NVRX_PERSISTENCE_MIN_REPORTS': 'y', 'NVRX_PEER_MIN_RANKS': 'z'}, {'peer_groups': 'mod:2'}, ValueError,
     'NVRX_PERSISTENCE_MIN_REPORTS must be an integer within [1, NVRX_SCORE_HISTORY]'),
    ({'NVRX_PEER_MIN_RANKS': 'z', 'NVRX_PEER_HISTORY': 'h'}, {'peer_groups': 'mod:2'}, ValueError,
     'NVRX_PEER_MIN_RANKS must be an integer >= 1'),
    ({'NVRX_PEER_HISTORY': 'h'}, {}, ValueError,
     'NVRX_PEER_HISTORY must be an integer: 0 (off) or 2..64 reports'),
    ({'NVRX_PEER_PERSISTENCE_MIN_REPORTS': 'y', 'NVRX_WORK_GROUPS': '2'}, {'peer_groups': 'mod:2', 'peer_history': 4}, ValueError,
     'NVRX_PEER_PERSISTENCE_MIN_REPORTS must be an integer within [1, NVRX_PEER_HISTORY]'),
    ({'NVRX_WORK_GROUPS': '2', 'NVRX_PACE_PEER_GROUPS': '2'}, {}, ValueError,
     "NVRX_WORK_GROUPS must be 0 or 1, got '2'"),
    ({'NVRX_WORK_COUNT_TOL': 'a', 'NVRX_WORK_MAX_UNLIKE': 'b'}, {'work_groups': True}, ValueError,
     "NVRX_WORK_COUNT_TOL must be a number, got 'a'"),
    ({'NVRX_WORK_MAX_UNLIKE': 'b'}, {'peer_groups': 'auto'}, ValueError,
     "NVRX_WORK_MAX_UNLIKE must be a number, got 'b'"),
    ({'NVRX_PACE_PEER_GROUPS': '2', 'NVRX_ROBUST_PEER_GROUPS': '2'}, {}, ValueError,
     "NVRX_PACE_PEER_GROUPS must be 0 or 1, got '2'"),
    ({'NVRX_ROBUST_PEER_GROUPS': 'yes', 'NVRX_SLACK_PEER_GROUPS': '2'}, {}, ValueError,
     "NVRX_ROBUST_PEER_GROUPS must be 0 or 1, got 'yes'"),
    ({'NVRX_SLACK_PEER_GROUPS': 'on', 'NVRX_ROW_PEER_GROUPS': '2'}, {}, ValueError,
     "NVRX_SLACK_PEER_GROUPS must be 0 or 1, got 'on'"),
    ({'NVRX_ROW_PEER_GROUPS': 'true', 'NVRX_NODE_SCORES': '2'}, {}, ValueError,
     "NVRX_ROW_PEER_GROUPS must be 0 or 1, got 'true'"),
    ({'NVRX_NODE_SCORES': '2', 'NVRX_NODE_PEER_GROUPS': '2'}, {}, ValueError,
     "NVRX_NODE_SCORES must be 0 or 1, got '2'"),
    ({'NVRX_NODE_PEER_GROUPS': '2', 'NVRX_PEER_ATTRIBUTION': 'x'}, {}, ValueError,
     "NVRX_NODE_PEER_GROUPS must be 0 or 1, got '2'"),
    ({'NVRX_PEER_ATTRIBUTION': 'x'}, {}, ValueError,
     'NVRX_PEER_ATTRIBUTION must be an integer: 0 (off) or 1..16'),
    # (what the environment switched on is handed to the generator, which says what it misses)
    ({'NVRX_PEER_TRENDS': '1'}, {}, ValueError,
     'peer_trends needs a peer history of at least 4 reports (peer_history within [4, 64]), got peer_history=0'),
    ({'NVRX_PEER_MIN_RANKS': '0'}, {'peer_groups': 'mod:2'}, ValueError,
     'peer_min_ranks must be an integer >= 1, got 0'),
    ({'NVRX_TAIL_QUANTILE': 'fast'}, {}, ValueError,
     "tail_quantile must be a number: 0 (off) or within [0.5, 0.999999], got 'fast'"),
]

# the generator's option attributes, and what they are with every option off (the others are absent then)
OPTION_ATTRS = (
    "asynchronous", "kernel_attribution", "tail_q_ppm", "robust_scores", "robust_min_ranks", "robust_floor", "peer_groups",
    "peer_min_ranks", "work_groups", "work_count_tol", "work_max_unlike", "work_max_unlike_ppm", "pace_scores", "pace_min_ranks",
    "pace_min_columns", "pace_min_effect", "pace_min_breadth", "pace_peer_groups", "robust_peer_groups", "node_scores",
    "node_groups", "node_min_members", "node_min_nodes", "node_min_columns", "node_min_effect", "node_min_breadth",
    "node_min_agree", "node_peer_groups", "onset_seg_ppm", "onset_min_strength", "period_max", "period_min_strength",
    "episode_len_ppm", "episode_min_strength", "ramp_seg_ppm", "ramp_min_strength", "stall_ratio_ppm", "stall_min_z",
    "stall_min_share", "score_history", "persistence_min_reports", "persistence_thresholds", "score_trends", "trend_min_reports",
    "trend_min_tau", "trend_horizon", "peer_history", "peer_persistence_min_reports", "peer_persistence_thresholds",
    "peer_trends", "peer_trend_horizon", "peer_attribution", "collective_slack", "slack_min_ranks", "slack_min_share",
    "slack_max_ratio", "slack_peer_groups", "row_peer_groups")
ALL_OFF = {
    'asynchronous': False, 'collective_slack': False, 'episode_len_ppm': 0, 'kernel_attribution': 0, 'node_groups': None,
    'node_peer_groups': False, 'node_scores': False, 'onset_seg_ppm': 0, 'pace_peer_groups': False, 'pace_scores': False,
    'peer_attribution': 0, 'peer_groups': None, 'peer_history': 0, 'peer_trends': False, 'period_max': 0, 'ramp_seg_ppm': 0,
    'robust_peer_groups': False, 'robust_scores': False, 'row_peer_groups': False, 'score_history': 0, 'score_trends': False,
    'slack_peer_groups': False, 'stall_ratio_ppm': 0, 'tail_q_ppm': 0, 'work_groups': False}
_PEERS = {'peer_groups': ('mod', 2), 'peer_min_ranks': 2}
_PACE = {'pace_scores': True, 'pace_min_ranks': 4, 'pace_min_columns': 8, 'pace_min_effect': 0.03, 'pace_min_breadth': 0.9}
_ROBUST = {'robust_scores': True, 'robust_min_ranks': 4, 'robust_floor': 0.02}
_SLACK = {'collective_slack': True, 'slack_min_ranks': 4, 'slack_min_share': 0.05, 'slack_max_ratio': 0.25}
_NODE = {'node_scores': True, 'node_min_members': 2, 'node_min_nodes': 3, 'node_min_columns': 8, 'node_min_effect': 0.03,
         'node_min_breadth': 0.9, 'node_min_agree': 0.75}
# (the group, the keywords with it on, the keywords that switch it on -- left out for "off" --, and what the generator's
# option attributes are beyond ALL_OFF with the group on and with it off)
GROUP_CASES = [
    ('peer_groups', {'peer_groups': 'mod:2', 'peer_min_ranks': 3}, ('peer_groups',),
     {'peer_groups': ('mod', 2), 'peer_min_ranks': 3}, {}),
    ('peer_history', {'peer_groups': 'mod:2', 'peer_history': 8, 'peer_persistence_min_reports': 4,
                      'peer_persistence_thresholds': (0.6, 0.7), 'peer_trends': True}, ('peer_history', 'peer_trends'),
     {**_PEERS, 'peer_history': 8, 'peer_persistence_min_reports': 4, 'peer_persistence_thresholds': (0.6, 0.7),
      'peer_trends': True, 'trend_min_reports': 6, 'trend_min_tau': 0.6, 'peer_trend_horizon': 8}, _PEERS),
    ('work_groups', {'work_groups': True, 'work_count_tol': 0.5, 'work_max_unlike': 0.2}, ('work_groups',),
     {'work_groups': True, 'work_count_tol': 0.5, 'work_max_unlike': 0.2, 'work_max_unlike_ppm': 200000}, {}),
    ('peer_groups_auto', {'peer_groups': 'auto', 'work_count_tol': 0.5, 'work_max_unlike': 0.2}, ('peer_groups',),
     {'peer_groups': 'auto', 'peer_min_ranks': 2, 'work_groups': True, 'work_count_tol': 0.5, 'work_max_unlike': 0.2,
      'work_max_unlike_ppm': 200000}, {}),
    ('pace_scores', {'pace_scores': True, 'pace_min_ranks': 2, 'pace_min_columns': 4, 'pace_min_effect': 0.05,
                     'pace_min_breadth': 0.8}, ('pace_scores',),
     {'pace_scores': True, 'pace_min_ranks': 2, 'pace_min_columns': 4, 'pace_min_effect': 0.05, 'pace_min_breadth': 0.8}, {}),
    ('pace_peer_groups', {'pace_scores': True, 'peer_groups': 'mod:2', 'pace_peer_groups': True}, ('pace_peer_groups',),
     {**_PEERS, **_PACE, 'pace_peer_groups': True}, {**_PEERS, **_PACE}),
    ('robust_peer_groups', {'robust_scores': True, 'peer_groups': 'mod:2', 'robust_peer_groups': True}, ('robust_peer_groups',),
     {**_PEERS, **_ROBUST, 'robust_peer_groups': True}, {**_PEERS, **_ROBUST}),
    ('slack_peer_groups', {'collective_slack': True, 'peer_groups': 'mod:2', 'slack_peer_groups': True}, ('slack_peer_groups',),
     {**_PEERS, **_SLACK, 'slack_peer_groups': True}, {**_PEERS, **_SLACK}),
    ('row_peer_groups', {'tail_quantile': 0.9, 'peer_groups': 'mod:2', 'row_peer_groups': True}, ('row_peer_groups',),
     {**_PEERS, 'tail_q_ppm': 900000, 'row_peer_groups': True}, {**_PEERS, 'tail_q_ppm': 900000}),
    ('node_scores', {'node_scores': True, 'node_groups': 'block:2', 'node_min_members': 1, 'node_min_nodes': 2,
                     'node_min_columns': 4, 'node_min_effect': 0.05, 'node_min_breadth': 0.8, 'node_min_agree': 0.5},
     ('node_scores',),
     {'node_scores': True, 'node_groups': ('block', 2), 'node_min_members': 1, 'node_min_nodes': 2, 'node_min_columns': 4,
      'node_min_effect': 0.05, 'node_min_breadth': 0.8, 'node_min_agree': 0.5}, {}),
    ('node_peer_groups', {'node_scores': True, 'peer_groups': 'mod:2', 'node_peer_groups': True}, ('node_peer_groups',),
     {**_PEERS, **_NODE, 'node_peer_groups': True}, {**_PEERS, **_NODE}),
    ('peer_attribution', {'peer_groups': 'mod:2', 'peer_attribution': 3}, ('peer_attribution',),
     {**_PEERS, 'peer_attribution': 3}, _PEERS),
    ('ramp_detection', {'ramp_detection': True, 'ramp_min_segment': 0.1, 'ramp_min_strength': 0.7}, ('ramp_detection',),
     {'ramp_seg_ppm': 100000, 'ramp_min_strength': 0.7}, {}),
    ('stall_detection', {'stall_detection': True, 'stall_min_ratio': 2, 'stall_min_z': 4.0, 'stall_min_share': 0.05},
     ('stall_detection',), {'stall_ratio_ppm': 2000000, 'stall_min_z': 4.0, 'stall_min_share': 0.05}, {}),
]


@pytest.fixture
def use_backend():
    from nvrx_straggler import backend

    try:
        yield backend.set_backend
    finally:
        backend.set_backend(None)


@pytest.mark.parametrize("which,options,kind,message", CONSTRUCTOR_CASES)
def test_the_constructor_reports_the_first_bad_argument_word_for_word(use_backend, which, options, kind, message):
    from nvrx_straggler.reporting import ReportGenerator

    use_backend({None: lambda: None, "bare": _Bare, "full": FullOracleBackend, "peers": _Peers}[which]())
    options = dict(options)
    with pytest.raises(kind) as raised:
        ReportGenerator(options.pop("scores_to_compute", ["relative_perf_scores"]), node_name="n", **options)
    assert type(raised.value) is kind and str(raised.value) == message


@pytest.mark.parametrize("env,options,kind,message", DETECTOR_CASES)
def test_the_detector_reports_the_first_bad_variable_word_for_word(use_backend, monkeypatch, env, options, kind, message):
    import os

    from nvrx_straggler import Detector

    for name in [n for n in os.environ if n.startswith("NVRX_")]:
        monkeypatch.delenv(name)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    use_backend(_Checker())
    try:
        with pytest.raises(kind) as raised:
            Detector.initialize(node_name="n0", **options)
        assert type(raised.value) is kind and str(raised.value) == message and not Detector.initialized
    finally:
        if Detector.initialized:
            Detector.shutdown()


def _options_of(reporter):
    return {k: tuple(v) if isinstance(v, tuple) else v for k, v in vars(reporter).items() if k in OPTION_ATTRS}


@pytest.mark.parametrize("group,options,switches,on,off", GROUP_CASES, ids=[c[0] for c in GROUP_CASES])
def test_detector_and_folded_job_hand_a_group_on_when_it_is_on_and_leave_it_out_when_off(use_backend, monkeypatch, group, options,
                                                                                        switches, on, off):
    import os

    from nvrx_straggler import Detector
    from nvrx_straggler.folded import FoldedJob

    for name in [n for n in os.environ if n.startswith("NVRX_")]:
        monkeypatch.delenv(name)
    use_backend(_Checker())
    for keywords, want in ((options, on), ({k: v for k, v in options.items() if k not in switches}, off)):
        want = {**ALL_OFF, **want}
        Detector.initialize(node_name="n0", **keywords)
        try:
            assert _options_of(Detector.reporter) == want, (group, "Detector")
        finally:
            Detector.shutdown()
        job = FoldedJob(total_ranks=2, sections=1, ring_cap=16, **keywords)
        try:
            assert _options_of(job.reporter) == want, (group, "FoldedJob")
        finally:
            job.close()
