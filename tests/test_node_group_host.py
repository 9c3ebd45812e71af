"""Node scores per peer group without a GPU: the option, the cell resolver, the argument checks."""
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = ["relative_perf_scores"]


@pytest.mark.parametrize("options,missing", [({"node_scores": True}, "peer_groups is not set"),
                                             ({"peer_groups": "block:4"}, "node_scores is not set"),
                                             ({}, "node_scores and peer_groups are not set")])
def test_the_option_says_what_it_misses(options, missing):
    from nvrx_straggler.reporting import ReportGenerator

    with pytest.raises(ValueError, match="node_peer_groups needs node_scores and peer_groups; " + missing):
        ReportGenerator(REL, node_peer_groups=True, **options)


@pytest.mark.parametrize("peer_groups", ["block:4", "auto"])
def test_the_grouped_step_takes_the_node_steps_place(peer_groups):
    from nvrx_straggler.reporting import ReportGenerator

    for on, step in ((False, ("node_scores", "report_node")), (True, ("node_peer_groups", "report_node_group"))):
        gen = ReportGenerator(REL, node_scores=True, node_groups="block:2", peer_groups=peer_groups, node_peer_groups=on)
        assert gen.node_peer_groups is on and gen._cells_resolved is None
        assert [x for x in gen._one_call_needs if x[0] != "work_groups"] == [("peer_groups", "report_peer"), step]
        gen.close()


def test_the_environment_variable_is_the_detectors_default(monkeypatch):
    from node_oracle_backend import NodeOracleBackend
    from nvrx_straggler import Detector, backend

    class Backend(NodeOracleBackend):  # the CPU checker, which the option asks for the grouped step (no report runs here)
        node_group_score = None

    monkeypatch.setattr(backend, "_backend", Backend())
    both = dict(node_name="n0", node_scores=True, node_groups="block:2", peer_groups="mod:2")
    for env, arg, want in (("1", None, True), ("1", False, False), ("0", None, False), ("", None, False), (None, True, True)):
        monkeypatch.delenv("NVRX_NODE_PEER_GROUPS", raising=False) if env is None else monkeypatch.setenv("NVRX_NODE_PEER_GROUPS", env)
        Detector.initialize(**both, **({} if arg is None else {"node_peer_groups": arg}))
        try:
            assert Detector.reporter.node_peer_groups is want, (env, arg)
        finally:
            Detector.shutdown()
    monkeypatch.setenv("NVRX_NODE_PEER_GROUPS", "yes")
    with pytest.raises(ValueError, match="NVRX_NODE_PEER_GROUPS must be 0 or 1"):
        Detector.initialize(**both)
    monkeypatch.setenv("NVRX_NODE_PEER_GROUPS", "1")
    with pytest.raises(ValueError, match="node_peer_groups needs node_scores and peer_groups; node_scores and peer_groups are not set"):
        Detector.initialize(node_name="n0")
    assert not Detector.initialized


# (node of each rank, peer group of each rank) -> the array's parts, written out by hand
LAYOUTS = {
    "two stages of two nodes": ([0, 0, 1, 1, 2, 2, 3, 3], [0, 0, 0, 0, 1, 1, 1, 1], dict(
        cell=[0, 0, 1, 1, 2, 2, 3, 3], members=list(range(8)), cstart=[0, 2, 4, 6, 8], gstart=[0, 2, 4], nstart=[0, 1, 2, 3, 4],
        ncells=[0, 1, 2, 3], cgroup=[0, 0, 1, 1], maxima=(2, 2, 1))),
    # node "b" hosts ranks of both groups; cells by (group, node): (x, a) (x, b) (y, b) (y, c)
    "a node spanning two groups": (["a", "a", "b", "b", "b", "c"], ["x", "x", "x", "y", "y", "y"], dict(
        cell=[0, 0, 1, 2, 2, 3], members=list(range(6)), cstart=[0, 2, 3, 5, 6], gstart=[0, 2, 4], nstart=[0, 1, 3, 4],
        ncells=[0, 1, 2, 3], cgroup=[0, 0, 1, 1], maxima=(2, 2, 2))),
    # tensor parallelism of 2 inside a box: the groups interleave, so members is no identity and a node's cells are not adjacent
    "interleaved groups": ([0, 0, 0, 0, 1, 1], [0, 1, 0, 1, 0, 1], dict(
        cell=[0, 2, 0, 2, 1, 3], members=[0, 2, 4, 1, 3, 5], cstart=[0, 2, 3, 5, 6], gstart=[0, 2, 4], nstart=[0, 2, 4],
        ncells=[0, 2, 1, 3], cgroup=[0, 0, 1, 1], maxima=(2, 2, 2))),
}


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_resolver_builds_the_array_the_header_states(layout):
    from nvrx_straggler import _native
    from nvrx_straggler.backend import NodeCells, PeerGroups

    node_of, group_of, want = LAYOUTS[layout]
    cells = NodeCells(PeerGroups(node_of), PeerGroups(group_of))
    C, Gp, Gn = cells.G
    assert (C, Gp, Gn) == (len(want["cgroup"]), len(set(group_of)), len(set(node_of))) and cells.maxima == want["maxima"]
    parts = [want["cell"], want["members"], want["cstart"], want["gstart"], want["nstart"], want["ncells"], want["cgroup"],
             cells.peers.group.tolist()]
    assert cells.host.dtype == np.int32 and cells.host.tolist() == sum(parts, [])
    assert cells.host.size == _native.node_group_cells_len(len(node_of), C, Gp, Gn)


def test_more_cells_than_the_kernels_take_are_refused_and_a_change_of_either_side_resolves_again():
    from nvrx_straggler import _native
    from nvrx_straggler.backend import NodeCells, PeerGroups
    from nvrx_straggler.reporting import ReportGenerator

    R = _native.PEER_MAX_GROUPS + 2
    with pytest.raises(ValueError, match=f"node_peer_groups: {R} cells"):
        NodeCells(PeerGroups([r // 2 for r in range(R)]), PeerGroups([r % 2 for r in range(R)]))
    gen = ReportGenerator(REL, node_scores=True, node_groups="block:2", peer_groups="block:4", node_peer_groups=True)
    nodes, peers = PeerGroups([0, 0, 1, 1]), PeerGroups([0, 0, 0, 0])
    assert gen._cells_for(nodes, peers) is gen._cells_for(nodes, peers) is not gen._cells_for(nodes, PeerGroups([0, 0, 0, 0]))
    gen.close()


def test_the_argument_checks_run_clean_under_the_host_sanitizers():
    out = subprocess.run(["make", "-C", os.path.join(REPO, "nvidia-resiliency-ext_amd", "csrc"), "node-group-args-check"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "node_group_args_check: 0 failure(s)" in out.stdout
