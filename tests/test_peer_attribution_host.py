"""Peer attribution without a GPU: the argument checks, the option, the step's place in the follow-up order, and that a
generator with the option off never asks the backend for it."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = ["relative_perf_scores"]


def test_the_argument_checks_run_clean_under_the_host_sanitizers():
    out = subprocess.run(["make", "-C", os.path.join(REPO, "nvidia-resiliency-ext_amd", "csrc"), "peer-attribute-args-check"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "peer_attribute_args_check: 0 failure(s)" in out.stdout


@pytest.mark.parametrize("scores,options,says", [
    (REL, {}, "peer_attribution=3 needs peer_groups"),
    (["individual_perf_scores"], {}, "peer_attribution=3 needs peer_groups .and with it relative_perf_scores."),
    (REL, {"peer_groups": "block:4", "peer_attribution": 17}, "peer_attribution must be 0"),
    (REL, {"peer_groups": "auto", "peer_attribution": True}, "peer_attribution must be 0")])
def test_the_option_says_what_is_wrong(scores, options, says):
    from nvrx_straggler.reporting import ReportGenerator

    with pytest.raises(ValueError, match=says):
        ReportGenerator(scores, **dict({"peer_attribution": 3}, **options))


def test_the_environment_value_must_be_an_integer(monkeypatch):
    from nvrx_straggler import Detector, backend
    from peer_oracle_backend import PeerOracleBackend

    monkeypatch.setattr(backend, "_backend", PeerOracleBackend())  # (a CPU backend: the Detector needs no device)
    monkeypatch.setenv("NVRX_PEER_ATTRIBUTION", "three")
    with pytest.raises(ValueError, match="NVRX_PEER_ATTRIBUTION must be an integer"):
        Detector.initialize(scores_to_compute=REL, node_name="n0")
    monkeypatch.setenv("NVRX_PEER_ATTRIBUTION", "17")
    with pytest.raises(ValueError, match="peer_attribution must be 0"):
        Detector.initialize(scores_to_compute=REL, node_name="n0", peer_groups="block:4")
    assert not Detector.initialized


@pytest.mark.parametrize("peer_groups", ["block:4", "auto"])
def test_the_step_sits_behind_the_peer_steps(peer_groups):
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(REL, peer_groups=peer_groups, peer_history=8, peer_trends=True, peer_attribution=16, pace_scores=True)
    assert gen.peer_attribution == 16 and gen._table_steps_on
    assert [x for x in gen._one_call_needs if x[0] != "work_groups"] == [
        ("peer_groups", "report_peer"), ("pace_scores", "report_pace"), ("peer_history", "report_peer_history"),
        ("peer_trends", "report_peer_trend"), ("peer_attribution=16", "report_peer_attribute")]
    gen.close()


def test_with_the_option_off_the_backend_is_never_asked(monkeypatch):
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator

    class Asked(Exception):
        pass

    def asked(self, *a, **kw):
        raise Asked

    for cls, name in ((backend.HipBackend, "peer_attribute"), (backend.HipRings, "report_peer_attribute"),
                      (backend.Workspace, "peer_attr_buffers")):
        assert callable(getattr(cls, name))
        monkeypatch.setattr(cls, name, property(asked))
    gen = ReportGenerator(REL, peer_groups="block:4")
    assert gen.peer_attribution == 0 and all(m != "report_peer_attribute" for _, m in gen._one_call_needs)
    ws = backend.Workspace.__new__(backend.Workspace)
    ws.settle_readers()  # (a workspace nothing ran on: no handle, no buffer, no call)
    assert ws._peer_attr_last is None and ws._peer_attr_buf is None
    gen.close()
