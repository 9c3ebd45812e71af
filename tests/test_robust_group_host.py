"""Robust scores per peer group without a GPU: the option, the C ABI's three spellings, the family record, the argument checks."""
import os
import subprocess
from ctypes import POINTER, c_float, c_int, c_void_p

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = ["relative_perf_scores"]


@pytest.mark.parametrize("options,missing", [({"robust_scores": True}, "peer_groups is not set"),
                                             ({"peer_groups": "block:4"}, "robust_scores is not set"),
                                             ({}, "robust_scores and peer_groups are not set")])
def test_the_option_says_what_it_misses(options, missing):
    from nvrx_straggler.reporting import ReportGenerator

    with pytest.raises(ValueError, match="robust_peer_groups needs robust_scores and peer_groups; " + missing):
        ReportGenerator(REL, robust_peer_groups=True, **options)


@pytest.mark.parametrize("peer_groups", ["block:4", "auto"])
def test_the_grouped_step_takes_the_robust_steps_place_behind_the_peer_step(peer_groups):
    from nvrx_straggler.reporting import ReportGenerator

    off = ReportGenerator(REL, robust_scores=True, peer_groups=peer_groups, pace_scores=True)
    on = ReportGenerator(REL, robust_scores=True, peer_groups=peer_groups, pace_scores=True, robust_peer_groups=True)
    assert off.robust_peer_groups is False and on.robust_peer_groups is True
    tail = [("peer_groups", "report_peer"), ("pace_scores", "report_pace")]
    assert [x for x in off._one_call_needs if x[0] != "work_groups"] == [("robust_scores", "report_robust")] + tail
    assert [x for x in on._one_call_needs if x[0] != "work_groups"] == [tail[0], ("robust_peer_groups", "report_robust_group"), tail[1]]
    off.close()
    on.close()


def test_the_header_the_bindings_and_the_word_count_agree():
    from nvrx_straggler import _native

    header = open(os.path.join(REPO, "include", "nvrx_straggler.h")).read()
    assert ("#define NVRX_ROBUST_GROUP_WORDS(G, n_ranks, K, S) (4 * (size_t)(G) * ((size_t)(K) + (S)) + (size_t)(n_ranks) * 2 * "
            "(1 + (size_t)(S)))") in header
    assert _native.robust_group_words(5, 3, 7, 2) == 4 * 5 * 9 + 3 * 2 * 3
    assert _native.robust_group_words(1, 8, 5, 2) == _native.robust_words(8, 5, 2)  # one group: the job-wide block
    symbols = {name: args for name, _, args in _native.SYMBOLS}
    assert symbols["nvrx_robust_group_score"] == [c_void_p, c_int, c_int, c_int, c_void_p] + [c_int] * 6 + [c_float, c_void_p, c_void_p]
    assert symbols["nvrx_report_robust_group"] == [c_void_p, POINTER(_native.ReportDesc), c_void_p] + [c_int] * 6 + [c_float, c_void_p]
    assert "int nvrx_robust_group_score(" in header and "int nvrx_report_robust_group(" in header


def test_the_family_record_stands_beside_the_five_and_cuts_the_headers_layout():
    from nvrx_straggler import table_families as tf
    from nvrx_straggler.backend import HipBackend, HipRings

    assert tuple(f.name for f in tf.FAMILIES) == ("robust", "peer", "pace", "pace_group", "node")
    assert tuple(f.name for f in tf.SLOTS) == ("robust", "peer", "pace", "node") and set(tf.BY_NAME) == {f.name for f in tf.FAMILIES}
    fam = tf.ROBUST_GROUP
    assert fam not in tf.FAMILIES and fam.name == "robust_group"
    assert (fam.slot, fam.groups, fam.max_size, fam.c_args[2:]) == ("robust", "peer", True, ("min_ranks", "min_peers", "floor_rel"))
    assert fam.params == ("min_ranks", "min_peers", "floor_rel") and fam.rank_args(3, 5, (4, 2, 0.02)) == (3, 5, 4, 2, 0.02)
    G, n, K, S = 3, 5, 4, 2
    cols, scores = fam.cut(np.arange(words := fam.n_words(G, n, K, S), dtype=np.uint32), G, n, K, S)
    assert cols.shape == (G, K + S, 4) and cols.dtype == np.uint32 and scores.shape == (n, 2, 1 + S) and scores.dtype == np.float32
    assert cols[2, 5, 3] == 4 * (2 * (K + S) + 5) + 3  # record (g, c) at 16-byte unit g * (K+S) + c
    assert scores.view(np.uint32)[4, 1, 2] == 4 * G * (K + S) + (4 * 2 + 1) * (1 + S) + 2 == words - 1
    assert callable(HipBackend.robust_group_score) and callable(HipBackend.robust_group_copy_out) and callable(HipRings.report_robust_group)


def test_the_argument_checks_run_clean_under_the_host_sanitizers():
    out = subprocess.run(["make", "-C", os.path.join(REPO, "nvidia-resiliency-ext_amd", "csrc"), "robust-group-args-check"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "robust_group_args_check: 0 failure(s)" in out.stdout
