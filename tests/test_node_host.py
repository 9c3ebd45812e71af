"""Node scores, host side, on the CPU checker backend (tests/node_oracle_backend.py): the NumPy restatement against the pace
scores' one (every rank its own node: word for word) and on a hand-worked table, what the GPU parity cases must hold, the
32-rank scenario of the feature's sketch (4 nodes of 8, 120 kernels, seeds 0, 1 and 2026) through ReportGenerator, how the
nodes are derived (``rank_to_node`` on gloo ranks without a further collective, ``node_groups`` in a folded job), the option's
plumbing through ReportGenerator / Detector / FoldedJob's keywords / the Lightning callback, that nothing is called with the
option off, lifetime and pickling, and that header, bindings and macro agree.

Bounds: everything here runs on the restatement itself, so records are compared exactly; the scenario's bands are worked out
where they are asserted."""
import copy
import inspect
import json
import math
import pickle

import numpy as np
import pytest

import node_cases
import node_workers as workers
from mp_util import run_ranks
from node_oracle_backend import CountingNodeBackend, NodeOracleBackend, node_scores_table
from pace_group_oracle_backend import pace_group_columns
from pace_oracle_backend import pace_scores_table

NAN_BITS = 0x7FC00000


@pytest.fixture
def cpu_backend():
    from nvrx_straggler import backend

    be = NodeOracleBackend()
    backend.set_backend(be)
    try:
        yield be
    finally:
        backend.set_backend(None)


def _groups(labels):
    from nvrx_straggler.backend import PeerGroups

    return PeerGroups(list(labels))


def _small_table(rng, R, K, S):
    KS = K + S
    T = np.zeros((R, 2 * KS + K + 1), dtype=np.float32)
    T[:, :KS] = rng.choice(np.array([0.0, 1.0, 2.0, 3.0, 4.0, 6.0, np.inf, -1.0, np.nan], dtype=np.float32), (R, KS),
                           p=[0.05, 0.2, 0.2, 0.15, 0.1, 0.1, 0.05, 0.1, 0.05])
    T[:, 2 * KS : 2 * KS + K] = rng.integers(1, 50, (R, K))
    return T


# ---- 1. the restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,K,S,min_nodes", [(1, 3, 0, 1), (2, 2, 2, 2), (5, 4, 3, 2), (6, 0, 5, 3), (7, 9, 1, 4), (9, 6, 6, 1)])
def test_every_rank_its_own_node_is_the_pace_restatement_word_for_word(R, K, S, min_nodes):
    rng = np.random.default_rng(R * 100 + K * 10 + S)
    g = _groups(range(R))
    for _ in range(10):
        T = _small_table(rng, R, K, S)
        first = int(rng.integers(0, R))
        n = int(rng.integers(1, R - first + 1))
        pairs, cols, nodes, ranks, terms = node_scores_table(T, K, S, g.host, R, 1, 1, min_nodes, first, n)
        wcols, wrecs, wterms = pace_scores_table(T, K, S, first, n, min_nodes)
        assert np.array_equal(cols, wcols) and np.array_equal(ranks, wrecs) and np.array_equal(terms, wterms)
        full = pace_scores_table(T, K, S, 0, R, min_nodes)[1]
        assert np.array_equal(nodes[:, :, :5], full[:, :, :5]) and (nodes[:, :, 5:] == 0).all()
        assert np.array_equal(pairs, pace_group_columns(T, K, S, g.host, R, 1, 1, 1))


def test_restatement_on_a_hand_worked_table():
    K, S = 2, 1
    T = np.zeros((7, 2 * (K + S) + K + 1), dtype=np.float32)
    # nodes by rank: a b a b a c c -- a = {0, 2, 4}, b = {1, 3}, c = {5, 6}
    T[:, 0] = [10.0, 100.0, 20.0, 200.0, 40.0, 7.0, 9.0]  # medians a 20, b 100, c 7: centre 20 (the lower median of three)
    T[:, 1] = [8.0, -1.0, -1.0, 50.0, 4.0, 7.0, -1.0]    # a: two present (4); b and c: one of two, below min(2, 2)
    T[:, 2] = [5.0, 5.0, 5.0, 6.0, 5.0, 5.0, 5.0]
    T[:, 6:8] = [[1.0, 2.0]] * 7
    g = _groups("ababacc")
    assert g.labels == ("a", "b", "c") and g.max_size == 3
    pairs, cols, nodes, ranks, _ = node_scores_table(T, K, S, g.host, g.G, g.max_size, 2, 2)
    pf, cf, nf, rf = pairs.view(np.float32), cols.view(np.float32), nodes.view(np.float32), ranks.view(np.float32)
    assert pf[:, 0, 0].tolist() == [20.0, 100.0, 7.0] and pairs[:, 0, 1:].tolist() == [[3, 1, 1], [2, 1, 0], [2, 1, 0]]
    assert pf[0, 1, 0] == 4.0 and (pairs[1:, 1, 0] == NAN_BITS).all() and pairs[:, 1, 1].tolist() == [2, 1, 1]
    assert pf[:, 2, 0].tolist() == [5.0, 5.0, 5.0]
    assert cols[:, 1:].tolist() == [[3, 1, 1], [1, 0, 0], [3, 0, 0]]
    assert cf[0, 0] == 20.0 and cols[1, 0] == NAN_BITS and cf[2, 0] == 5.0  # one node of two needed: no centre, counts written
    # node records: a is the centre, b five times slower, c faster; kernel 1 has no centre, so one eligible kernel each
    assert nf[:, 0, 0].tolist() == [1.0, np.float32(0.2), np.float32(20.0 / 7.0)] and nodes[:, 0, 2].tolist() == [1, 1, 1]
    assert nodes[:, 0, 3].tolist() == [0, 1, 0] and nodes[:, 0, 4].tolist() == [0, 0, 1] and (nodes[:, :, 5:] == 0).all()
    assert nf[:, 1, 0].tolist() == [1.0, 1.0, 1.0]
    # rank records against the nodes' centre: rank 3 (200 us against 20; its section 6 against 5)
    assert rf[3, 0, 0] == np.float32(0.1) and rf[3, 1, 0] == np.float32(5.0 / 6.0) and ranks[3, 0, 2:5].tolist() == [1, 1, 0]
    assert rf[3, 0, 5:].tolist() == [1.0, 1.0, np.float32(1.0 * (1 - 0.1))]
    # at min_nodes = 1 kernel 1 has a centre: a's 4
    cols1, nodes1 = node_scores_table(T, K, S, g.host, g.G, g.max_size, 2, 1)[1:3]
    assert cols1.view(np.float32)[1, 0] == 4.0 and nodes1[:, 0, 2].tolist() == [2, 1, 1]


@pytest.mark.parametrize("R,K,S,layout", node_cases.CASES)
def test_the_gpu_parity_cases_hold_what_the_gpu_test_relies_on(R, K, S, layout):
    """With the restatement alone: every case rates some node, holds a pair with data and no reference where a node has two
    members, and for three nodes or more a column with referenced nodes but fewer than ``min_nodes``."""
    labels = node_cases.labels_of(R, layout)
    g = _groups(labels)
    results = [node_scores_table(T, K, S, g.host, g.G, g.max_size, mm, mn)
               for T in node_cases.tables(R, K, S, labels) for mm, mn in node_cases.THRESHOLDS]
    node_cases.check_properties(node_cases.case_properties(results, g.G), labels)


# ---- 2. the sketch's scenario -------------------------------------------------------------------------------------------------
def _load(rings, rows, med):
    for lr in range(med.shape[0]):
        for k, row in enumerate(rows.values()):
            rings.push_many(row, np.full(workers.SAMPLES, med[lr, k], dtype=np.float32), lr=lr)


def _scenario_reports(be, med, **options):
    from nvrx_straggler.reporting import ReportGenerator

    R, K = med.shape
    gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=True, node_name="n", pace_scores=True, node_scores=True,
                          node_groups=f"block:{workers.PER_NODE}", **options)
    rings = be.make_rings(R, K, 256)
    rows = {name: rings.row_for(1, name) for name in workers.KERNEL_NAMES}
    try:
        for _ in range(2):  # the general path (_assemble), then the planned one
            _load(rings, rows, med)
            rep = gen.generate_report_from_rings(rings, {}, rows, local_ranks=R)
            rings.reset()
            yield rep
    finally:
        gen.close()


@pytest.mark.parametrize("emulate_fused", [False, True])
@pytest.mark.parametrize("seed", workers.SEEDS)
def test_the_scenario_names_node_2_alone_and_rank_5_as_off_pace_without_its_node(seed, emulate_fused):
    from nvrx_straggler import backend

    be = NodeOracleBackend(emulate_fused=emulate_fused)
    backend.set_backend(be)
    try:
        med = workers.scenario_medians(seed)
        R, K = med.shape
        for rep in _scenario_reports(be, med):
            # the pace rule on the same report: nine ranks, and no word on which of them are one incident
            assert workers.ranks_named(rep.identify_pace_stragglers()["straggler_gpus_relative"]) == [5] + workers.SLOW_NODE_RANKS
            found = rep.identify_node_stragglers()
            assert found["straggler_nodes"] == {workers.SLOW_NODE} and found["straggler_section_nodes"] == set()
            assert workers.ranks_named(found["ranks_off_pace_alone"]) == [workers.SLOW_RANK]
            assert {s.node for s in found["ranks_off_pace_alone"]} == {"n"} and found["section_ranks_off_pace_alone"] == set()
            t = rep.node_scores()
            json.dumps(t)
            assert t["params"] == {"min_members": 2, "min_nodes": 3, "min_columns": 8, "min_effect": 0.03, "min_breadth": 0.9,
                                   "min_agree": 0.75}
            assert t["nodes"] == {g: list(range(8 * g, 8 * g + 8)) for g in range(4)} and t["unrated_nodes"] == []
            assert t["node_of"] == {r: r // 8 for r in range(R)} and sorted(t["ranks"]) == list(range(R))
            assert sorted(t["kernels"]) == sorted(workers.KERNEL_NAMES) and t["section_columns"] == {}
            assert all(c["nodes"] == 4 and sorted(c["per_node"]) == [0, 1, 2, 3] and all(x["ranks"] == 8 for x in c["per_node"].values())
                       for c in t["kernels"].values())
            slow = t["node_scores"][workers.SLOW_NODE]
            # 1 / 1.04 = 0.9615; a node's median of eight entries with 1 % noise each, and the median of 120 such quotients,
            # lie well within 0.5 % of it
            assert 0.956 <= slow["gpu"]["pace"] <= 0.967 and slow["gpu"]["slower"] == K and slow["gpu"]["columns"] == K
            assert (slow["members_rated"], slow["members_off_pace"], slow["agree"]) == (8, 8, 1.0)
            assert "total_us" not in slow["gpu"]
            for g in set(range(4)) - {workers.SLOW_NODE}:
                d = t["node_scores"][g]
                assert 0.995 <= d["gpu"]["pace"] <= 1.005 and d["gpu"]["breadth"] < 0.9, (g, d)
                assert d["members_rated"] == 8 and d["members_off_pace"] == (1 if g == 0 else 0)
            # every kernel's centre is one of the nodes' medians: one node, one vote
            c = t["kernels"][workers.KERNEL_NAMES[0]]
            assert c["center"] in [x["median"] for x in c["per_node"].values()] and c["above"] + c["below"] == 3
            assert t["ranks"][workers.SLOW_RANK]["gpu"]["excess_us"] > 0
        assert be.node_calls == 2 and be.node_args == [(R, 4, 8, 2, 3, 0, R)] * 2
    finally:
        backend.set_backend(None)


def test_a_node_whose_members_do_not_agree_is_not_named(cpu_backend):
    """Five of node 2's eight ranks 6 % slower, three healthy: the node's lower median is a slow rank's value in every kernel,
    so its pace and breadth meet the rule -- but 5 of 8 members off pace is below ``node_min_agree`` = 0.75, and the five are
    handed back as ranks off pace on their own.  At ``min_agree`` 0.6 the same report names the node."""
    med = workers.scenario_medians(2026, slow_node_factor=1.06, slow_members=5)
    for rep in _scenario_reports(cpu_backend, med):
        t = rep.node_scores()["node_scores"][workers.SLOW_NODE]
        assert t["gpu"]["pace"] <= 0.97 and t["gpu"]["breadth"] >= 0.9 and t["gpu"]["columns"] == workers.KERNELS
        assert (t["members_rated"], t["members_off_pace"], t["agree"]) == (8, 5, 0.625)
        found = rep.identify_node_stragglers()
        assert found["straggler_nodes"] == set()
        assert workers.ranks_named(found["ranks_off_pace_alone"]) == [5] + workers.SLOW_NODE_RANKS[:5]
        relaxed = rep.identify_node_stragglers(min_agree=0.6)
        assert relaxed["straggler_nodes"] == {workers.SLOW_NODE} and workers.ranks_named(relaxed["ranks_off_pace_alone"]) == [5]


# ---- 3. where the nodes come from ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("emulate_fused", [False, True])
def test_nodes_come_from_rank_to_node_without_a_further_collective(emulate_fused):
    world = 4
    kw = dict(gather_on_rank0=True, emulate_fused=emulate_fused)
    on = run_ranks(workers.ring_reports_recorded, world, timeout=300, node_scores=True, **kw)
    off = run_ranks(workers.ring_reports_recorded, world, timeout=300, node_scores=False, **kw)
    for r in range(world):
        assert on[r]["calls"] == off[r]["calls"], r  # the same collectives, report by report
        assert off[r]["node_calls"] == 0 and on[r]["node_calls"] == (6 if r == 0 else 0) and on[r]["errors"] == []
        assert all(a == (world, 2, 2, 2, 1, 0, world) for a in on[r]["node_args"]), on[r]["node_args"]
        assert on[r]["fused"][0] is None and on[r]["fused"][-1] is emulate_fused  # the general path, then the plan
        for entry in on[r]["reports"]:
            if r != 0:
                assert entry["node"] is None
                continue
            t = entry["node"]
            assert entry["pickled_same"]
            assert t["nodes"] == {"host0": [0, 1], "host1": [2, 3]} and t["node_of"] == {x: f"host{x // 2}" for x in range(world)}
            assert sorted(t["ranks"]) == list(range(world)) and sorted(t["node_scores"]) == ["host0", "host1"]
            assert {"k0", "k1"} <= set(t["kernels"]) and "ncclDevKernel_z" not in t["kernels"]
            assert all(c["nodes"] == 2 and c["per_node"]["host1"]["ranks"] == 2 for n, c in t["kernels"].items() if n in ("k0", "k1"))


def test_a_rank_that_covers_only_itself_needs_node_groups_and_sees_its_own_agreement():
    world = 4
    # rank_to_node is gathered with gather_on_rank0 only: without it a rank knows its own node alone, and says so
    res = run_ranks(workers.ring_reports_recorded, world, timeout=300, gather_on_rank0=False)
    for r in range(world):
        assert res[r]["node_calls"] == 0 and len(res[r]["errors"]) == 6
        assert "rank_to_node names 1 of the job's 4 logical ranks" in res[r]["errors"][0] and "pass node_groups" in res[r]["errors"][0]
    res = run_ranks(workers.ring_reports_recorded, world, timeout=300, gather_on_rank0=False, node_groups="block:2")
    for r in range(world):
        assert res[r]["errors"] == [] and res[r]["node_calls"] == 6
        assert all(a == (world, 2, 2, 2, 1, r, 1) for a in res[r]["node_args"]), res[r]["node_args"]
        for entry in res[r]["reports"]:
            t = entry["node"]
            assert sorted(t["ranks"]) == [r] and t["nodes"] == {0: [0, 1], 1: [2, 3]} and sorted(t["node_scores"]) == [0, 1]
            # block C is whole; agree is over the one member this report covers, None for the other node
            assert t["node_scores"][r // 2]["members_rated"] <= 1 and t["node_scores"][1 - r // 2]["agree"] is None
            assert t["node_scores"][1 - r // 2]["gpu"]["columns"] >= 2


def test_nodes_in_a_folded_job_and_a_label_list_of_the_wrong_length(cpu_backend):
    from nvrx_straggler import Statistic as S
    from nvrx_straggler.reporting import ReportGenerator

    med = workers.scenario_medians(0, ranks=6, kernels=9)
    for spec, want in (("mod:2", {0: [0, 2, 4], 1: [1, 3, 5]}), (["x", "x", "y", "y", "y", "x"], {"x": [0, 1, 5], "y": [2, 3, 4]}),
                       (None, {"n": [0, 1, 2, 3, 4, 5]})):  # (folded: every logical rank inherits the process' node)
        gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=True, node_name="n", node_scores=True, node_groups=spec)
        rings = cpu_backend.make_rings(6, 9, 256)
        rows = {name: rings.row_for(1, name) for name in workers.KERNEL_NAMES[:9]}
        _load(rings, rows, med)
        t = gen.generate_report_from_rings(rings, {}, rows, local_ranks=6).node_scores()
        assert t["nodes"] == want and t["params"]["min_nodes"] == min(3, len(want))  # clamped to the job's nodes
        gen.close()
    gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=True, node_name="n", node_scores=True, node_groups=[0, 0, 1])
    summ = {S.MIN: 1.0, S.MAX: 2.0, S.MED: 1.5, S.AVG: 1.5, S.STD: 0.1, S.NUM: 4}
    with pytest.raises(ValueError, match="node_groups has 3 labels, the job has 1 logical ranks"):
        gen.generate_report({"sec": summ}, {"gemm": summ})
    gen.close()


def test_nodes_are_resolved_again_when_rank_to_node_changes(cpu_backend):
    from nvrx_straggler import Statistic as S
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=True, node_name="first", node_scores=True, node_min_columns=1)
    summ = {S.MIN: 1.0, S.MAX: 2.0, S.MED: 1.5, S.AVG: 1.5, S.STD: 0.1, S.NUM: 4}
    t = gen.generate_report({"sec": summ}, {"gemm": summ}).node_scores()
    assert t["nodes"] == {"first": [0]} and t["params"]["min_nodes"] == 1
    kept = gen._node_resolved
    gen.generate_report({"sec": summ}, {"gemm": summ})
    assert gen._node_resolved is kept  # (cold path: once per R and rank_to_node)
    gen.rank_to_node = {0: "second"}  # replaced, never edited, when it changes
    t = gen.generate_report({"sec": summ}, {"gemm": summ}).node_scores()
    assert t["nodes"] == {"second": [0]} and gen._node_resolved is not kept
    # one node of one rank: its own centre, pace 1, and the node record equals the rank's without the sums
    assert t["node_scores"]["second"]["gpu"] == {"pace": 1.0, "spread": 0.0, "columns": 1, "slower": 0, "faster": 0,
                                                 "breadth": 0.0, "members_rated": 1, "members_off_pace": 0, "agree": 0.0}
    assert t["ranks"][0]["gpu"]["total_us"] == 6.0
    gen.close()


# ---- 4. the option's values ---------------------------------------------------------------------------------------------------
def test_option_values(cpu_backend, monkeypatch):
    from nvrx_straggler import Detector
    from nvrx_straggler.folded import FoldedJob
    from nvrx_straggler.reporting import ReportGenerator

    rel = ["relative_perf_scores"]
    gen = ReportGenerator(rel, node_scores=True)
    assert gen.node_scores is True and gen.node_groups is None
    assert (gen.node_min_members, gen.node_min_nodes, gen.node_min_columns) == (2, 3, 8)
    assert (gen.node_min_effect, gen.node_min_breadth, gen.node_min_agree) == (0.03, 0.9, 0.75)
    assert ReportGenerator(rel).node_scores is False and ReportGenerator(rel, node_groups="bogus").node_groups is None  # off: unread
    assert ReportGenerator(rel, node_scores=True, node_groups="block:8").node_groups == ("block", 8)
    assert ReportGenerator(rel, node_scores=True, node_groups=np.array([1, 1, 0])).node_groups == (1, 1, 0)
    for bad, kind, text in (("block", ValueError, "node_groups must be 'block:N'"), ("mod:0", ValueError, "N must be at least 1"),
                            (7, TypeError, "node_groups must be"), ([1.5], TypeError, "node_groups labels must be int or str"),
                            ([], ValueError, "node_groups must have one label per logical rank, got none")):
        with pytest.raises(kind, match=text):
            ReportGenerator(rel, node_scores=True, node_groups=bad)
    for name in ("node_min_members", "node_min_nodes", "node_min_columns"):
        for bad in (0, -1, 1.5, True, "2"):
            with pytest.raises(ValueError, match=f"{name} must be an integer >= 1"):
                ReportGenerator(rel, node_scores=True, **{name: bad})
    for name, bads in (("node_min_effect", (-0.1, 1.0)), ("node_min_breadth", (0.0, 1.1)), ("node_min_agree", (0.0, 1.1))):
        for bad in bads:
            with pytest.raises(ValueError, match=f"{name} must be within"):
                ReportGenerator(rel, node_scores=True, **{name: bad})
    with pytest.raises(ValueError, match="must be numbers"):
        ReportGenerator(rel, node_scores=True, node_min_agree="most")
    with pytest.raises(ValueError, match="node_scores needs relative_perf_scores"):
        ReportGenerator(["individual_perf_scores"], node_scores=True)
    params = inspect.signature(FoldedJob.__init__).parameters
    defaults = {"node_scores": False, "node_groups": None, "node_min_members": 2, "node_min_nodes": 3, "node_min_columns": 8,
                "node_min_effect": 0.03, "node_min_breadth": 0.9, "node_min_agree": 0.75}
    for cls in (FoldedJob, ReportGenerator):
        params = inspect.signature(cls.__init__).parameters
        assert {k: params[k].default for k in defaults} == defaults, cls
    params = inspect.signature(Detector.initialize).parameters
    assert {k: params[k].default for k in defaults} == dict(defaults, node_scores=None)
    # the environment variables are the Detector's defaults, read only when the argument is None
    for env, arg, want in (("1", None, True), ("1", False, False), ("0", None, False), ("", None, False), (None, True, True),
                           (None, None, False)):
        if env is None:
            monkeypatch.delenv("NVRX_NODE_SCORES", raising=False)
        else:
            monkeypatch.setenv("NVRX_NODE_SCORES", env)
        Detector.initialize(node_name="n0", **({} if arg is None else {"node_scores": arg}))
        try:
            assert Detector.reporter.node_scores is want, (env, arg)
        finally:
            Detector.shutdown()
    monkeypatch.setenv("NVRX_NODE_SCORES", "yes")
    with pytest.raises(ValueError, match="NVRX_NODE_SCORES must be 0 or 1"):
        Detector.initialize(node_name="n0")
    assert not Detector.initialized
    monkeypatch.setenv("NVRX_NODE_SCORES", "1")
    for env, arg, want in (("mod:4", None, ("mod", 4)), ("mod:4", "block:2", ("block", 2)), ("", None, None), (None, None, None),
                           (None, [0], (0,)), ("7", None, (7,)), (" 3 ", [0], (0,))):  # (labels, as NVRX_PEER_GROUPS takes them)
        if env is None:
            monkeypatch.delenv("NVRX_NODE_GROUPS", raising=False)
        else:
            monkeypatch.setenv("NVRX_NODE_GROUPS", env)
        Detector.initialize(node_name="n0", node_min_agree=0.5, **({} if arg is None else {"node_groups": arg}))
        try:
            assert Detector.reporter.node_groups == want and Detector.reporter.node_min_agree == 0.5, (env, arg)
        finally:
            Detector.shutdown()
    monkeypatch.setenv("NVRX_NODE_GROUPS", "rack:4")
    with pytest.raises(ValueError, match="node_groups must be 'block:N'"):
        Detector.initialize(node_name="n0")
    assert not Detector.initialized
    monkeypatch.setenv("NVRX_NODE_GROUPS", "0,0,one")
    with pytest.raises(ValueError, match="NVRX_NODE_GROUPS must be 'block:N', 'mod:N' or a comma-separated list of integers"):
        Detector.initialize(node_name="n0")
    assert not Detector.initialized
    monkeypatch.setenv("NVRX_NODE_SCORES", "0")
    Detector.initialize(node_name="n0")  # (off: NVRX_NODE_GROUPS is not read)
    Detector.shutdown()


def test_option_needs_a_backend_with_node_score():
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator
    from pace_group_oracle_backend import PaceGroupOracleBackend

    backend.set_backend(PaceGroupOracleBackend())
    try:
        with pytest.raises(RuntimeError, match=r"no node scores \(backend.node_score\)"):
            ReportGenerator(["relative_perf_scores"], node_scores=True)
        ReportGenerator(["relative_perf_scores"], pace_scores=True)
    finally:
        backend.set_backend(None)


# ---- 5. off: nothing is called; on: the arguments passed -----------------------------------------------------------------------
@pytest.mark.parametrize("emulate_fused,asynchronous", [(False, False), (True, False), (True, True)])
def test_option_off_calls_nothing(emulate_fused, asynchronous):
    from nvrx_straggler import Detector
    from nvrx_straggler import Statistic as S
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator

    be = CountingNodeBackend(emulate_fused=emulate_fused)
    backend.set_backend(be)
    try:
        gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=True, node_name="n",
                              asynchronous=asynchronous, pace_scores=True, pace_min_ranks=1, node_groups="block:1")
        assert gen.node_scores is False and gen._node_resolved is None
        summ = {S.MIN: 1.0, S.MAX: 2.0, S.MED: 1.5, S.AVG: 1.5, S.STD: 0.1, S.NUM: 4}
        rep = gen.generate_report({"sec": summ}, {"k": summ})
        assert rep.node_scores() == {} and pickle.loads(pickle.dumps(rep)).node_scores() == {} and "_node" not in rep.__dict__
        assert rep.identify_node_stragglers() == {"straggler_nodes": set(), "straggler_section_nodes": set(),
                                                  "ranks_off_pace_alone": set(), "section_ranks_off_pace_alone": set()}
        rings = be.make_rings(1, 8, 16)
        krow, srow = rings.row_for(1, "kern"), rings.row_for(0, "sec")
        for i in range(3):
            rings.push_many(krow, [1.0 + i, 2.0, 3.0])
            rings.push_many(srow, [5.0, 6.0])
            rep = gen.generate_report_from_rings(rings, {"sec": srow}, {"kern": krow})
            rings.reset()
            assert rep.node_scores() == {} and rep.pace_scores()
        assert gen._ring_plan is not None and gen._node_resolved is None
        gen.close()
        Detector.initialize(scores_to_compute="all", gather_on_rank0=True, node_name="n0", asynchronous=asynchronous)
        try:
            for t in range(3):
                for name, value in (("a", 2.0 + t), ("b", 4.0)):
                    with Detector.detection_section(name, profile_cuda=False):
                        pass
                    sec = Detector.custom_sections[name]
                    sec.cpu_elapsed_times.clear()
                    sec.cpu_elapsed_times.extend(np.full(5, value, dtype=np.float32))
                assert Detector.generate_report().node_scores() == {}
        finally:
            Detector.shutdown()
        assert be.node_calls == 0 and be.pace_calls > 0
    finally:
        backend.set_backend(None)


def test_the_product_workspace_holds_no_node_buffer_until_asked():
    """``Workspace``'s table-family state is class-level None: a workspace no node step ran on has no node buffer and nothing
    to settle -- and the same holds of the robust, peer and pace slots."""
    from nvrx_straggler.backend import Workspace

    assert Workspace._table_state is None
    ws = Workspace.__new__(Workspace)
    for slot in ("node", "robust", "peer", "pace"):
        getattr(ws, slot + "_settle")()  # (nothing in flight: no call into a backend)
        assert "_table_state" not in ws.__dict__ and ws._table_state is None, slot  # no buffer, no step in flight
    ws.settle_readers()
    assert ws.__dict__ == {}


@pytest.mark.parametrize("emulate_fused,asynchronous", [(False, False), (True, False), (True, True)])
def test_all_three_attachment_sites_and_the_arguments_passed(emulate_fused, asynchronous):
    from nvrx_straggler import Statistic as S
    from nvrx_straggler import backend
    from nvrx_straggler.reporting import ReportGenerator

    be = NodeOracleBackend(emulate_fused=emulate_fused)
    backend.set_backend(be)
    try:
        order = []
        for name in ("robust_score", "pace_score", "node_score"):
            def spy(*a, _name=name, _inner=getattr(be, name), **kw):
                order.append(_name)
                return _inner(*a, **kw)
            setattr(be, name, spy)
        gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=True, node_name="n",
                              asynchronous=asynchronous, pace_scores=True, robust_scores=True, node_scores=True,
                              node_min_members=3, node_min_nodes=5, node_min_columns=1)
        # (a) the dict-input report: _assemble
        summ = {S.MIN: 1.0, S.MAX: 2.0, S.MED: 1.5, S.AVG: 1.5, S.STD: 0.1, S.NUM: 4}
        t = gen.generate_report({"sec": summ}, {"gemm": summ}).node_scores()
        assert order == ["robust_score", "pace_score", "node_score"]
        assert t["kernels"] == {"gemm": {"center": 1.5, "nodes": 1, "above": 0, "below": 0,
                                         "per_node": {"n": {"median": 1.5, "ranks": 1}}}}
        assert t["section_columns"]["sec"]["center"] == 1.5 and t["unrated_nodes"] == []
        assert t["ranks"][0]["gpu"] == {"pace": 1.0, "spread": 0.0, "columns": 1, "slower": 0, "faster": 0, "breadth": 0.0,
                                        "total_us": 6.0, "slower_us": 0.0, "excess_us": 0.0}
        assert be.node_args == [(1, 1, 1, 3, 1, 0, 1)]  # min_members as given, min_nodes clamped to the one node
        # (b) ring reports: _assemble for the first, then the planned path -- stepwise, or one call through the rings
        rings = be.make_rings(1, 8, 16)
        kernel_rows = {"gemm": rings.row_for(1, "gemm")}
        section_rows = {"sec": rings.row_for(0, "sec")}
        before = be.node_calls
        for w in range(4):
            v = np.arange(1, 12, dtype=np.float32) * (w + 1)
            rings.push_many(kernel_rows["gemm"], v)
            rings.push_many(section_rows["sec"], v[::-1] + 0.5)
            t = gen.generate_report_from_rings(rings, section_rows, kernel_rows).node_scores()
            rings.reset()
            assert t["kernels"]["gemm"]["center"] == 6.0 * (w + 1) and t["section_columns"]["sec"]["per_node"]["n"]["median"] == 6.0 * (w + 1) + 0.5
            assert t["node_scores"]["n"]["gpu"]["pace"] == 1.0 and t["ranks"][0]["gpu"]["total_us"] == float(np.float32(v.sum()))
        assert gen._ring_plan is not None and gen._ring_plan.fused == emulate_fused
        assert be.node_calls - before == 4 and be.node_args[-1] == (1, 1, 1, 3, 1, 0, 1)
        assert be.node_calls - order.count("node_score") == (3 if emulate_fused else 0)  # through the rings' report_node
        gen.close()
    finally:
        backend.set_backend(None)


# ---- 6. lifetime and pickling -------------------------------------------------------------------------------------------------
def test_a_held_report_keeps_its_node_scores_and_reports_travel(cpu_backend):
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=True, node_name="n", node_scores=True)
    rings = cpu_backend.make_rings(1, 8, 16)
    kernel_rows = {"gemm": rings.row_for(1, "gemm")}
    section_rows = {"sec": rings.row_for(0, "sec")}
    held = []
    for w in range(4):
        v = np.arange(1, 12, dtype=np.float32) * (w + 1)
        rings.push_many(kernel_rows["gemm"], v)
        rings.push_many(section_rows["sec"], v[::-1] + 0.5)
        held.append(gen.generate_report_from_rings(rings, section_rows, kernel_rows))
        rings.reset()
    handles = cpu_backend.node_handles
    assert cpu_backend.node_calls == 4 and all(h.reads == 0 for h in handles)  # generate_report reads nothing
    for w in (1, 0, 3, 2):  # a report held across the next two is still its own
        t = held[w].node_scores()
        assert handles[w].reads == 1
        assert t["kernels"]["gemm"]["center"] == 6.0 * (w + 1) and t["section_columns"]["sec"]["center"] == 6.0 * (w + 1) + 0.5
        assert held[w].node_scores() == t and handles[w].reads == 1
        for clone in (pickle.loads(pickle.dumps(held[w])), copy.deepcopy(held[w])):
            assert json.dumps(clone.node_scores()) == json.dumps(t)
            assert clone.identify_node_stragglers() == held[w].identify_node_stragglers()
            assert isinstance(clone.__dict__["_node"], dict)  # materialised
    t = held[0].node_scores()
    t["kernels"].clear()
    t["nodes"]["n"].clear()
    t["node_scores"]["n"]["gpu"].clear()
    again = held[0].node_scores()
    assert again["kernels"] and again["nodes"] == {"n": [0]} and again["node_scores"]["n"]["gpu"]
    gen.close()


# ---- 7. the lane declines, as for pace scores ---------------------------------------------------------------------------------
def test_lane_declines_while_the_option_is_on():
    from types import SimpleNamespace

    from nvrx_straggler import straggler

    class Reached(Exception):
        pass

    class Manager:
        is_initialized = True

        @property
        def cupti_ext(self):
            raise Reached  # what _Lane.build asks for right after its option checks

    def det(on):
        # node_scores is the only option that is ever on: with it off, build gets past every option check
        reporter = SimpleNamespace(_ring_plan=SimpleNamespace(fused=True, ws=None), world_size=1, _exchanged=lambda: True,
                                   _direct=None, asynchronous=False, kernel_attribution=0, tail_q_ppm=0, node_scores=on)
        rings = SimpleNamespace(lib=SimpleNamespace(nvrx_window_report=object()))
        return SimpleNamespace(_rings=rings, reporter=reporter, _cupti_manager=Manager(), _pending_region_switch=None)

    with pytest.raises(Reached):
        straggler._Lane.build(det(False))
    assert straggler._Lane.build(det(True)) is None


# ---- 8. the Lightning callback ------------------------------------------------------------------------------------------------
def test_callback_warns_once_per_report_of_a_node_off_pace_and_never_halts_for_it(monkeypatch):
    import callback_script
    import nvrx_straggler
    from nvidia_resiliency_ext.ptl_resiliency import StragglerDetectionCallback
    from nvrx_straggler.reporting import Report

    healthy = callback_script._scores(8)
    base = {k: v for k, v in callback_script.reports(8)[1].items() if not k.startswith("gpu_")}
    # per report: the paces of node1's ranks 4..7 (the node's own is their median); {} = everybody healthy
    sequence = [None, {4: 0.961, 5: 0.960, 6: 0.962, 7: 0.961}, None, {}, {6: 0.95}, {4: 0.96, 5: 0.96, 6: 0.96, 7: 0.96}]

    def part(pace, slower):
        return {"pace": pace, "spread": 0.007, "columns": 120, "slower": slower, "faster": 120 - slower, "breadth": slower / 120}

    none = {"pace": float("nan"), "spread": float("nan"), "columns": 0, "slower": 0, "faster": 0, "breadth": None}

    def node_of(slow):
        ranks = {r: {"gpu": dict(part(slow.get(r, 1.0), 120 if r in slow else 55), total_us=1e6, slower_us=5e5, excess_us=0.0),
                     "sections": dict(none)} for r in range(8)}
        whole = len(slow) == 4
        nodes = {"node0": {"gpu": part(1.0, 50), "sections": dict(none)},
                 "node1": {"gpu": part(0.961 if whole else 1.0, 120 if whole else 60), "sections": dict(none)}}
        t = {"nodes": {"node0": [0, 1, 2, 3], "node1": [4, 5, 6, 7]}, "node_of": {r: f"node{r // 4}" for r in range(8)},
             "kernels": {}, "section_columns": {}, "node_scores": nodes, "ranks": ranks, "unrated_nodes": [],
             "params": {"min_members": 2, "min_nodes": 2, "min_columns": 8, "min_effect": 0.03, "min_breadth": 0.9, "min_agree": 0.75}}
        for lab, d in nodes.items():
            off = sum(1 for r in t["nodes"][lab] if r in slow)
            d.update(members_rated=4, members_off_pace=off, agree=off / 4)
        return t

    def scripted(n_ranks):
        return [None if e is None else dict(base, gpu_relative_perf_scores=healthy, gpu_individual_perf_scores=healthy,
                                            node=node_of(e)) for e in sequence]

    def make_report(node=None, **fields):
        rep = Report(**fields)
        rep.__dict__["_node"] = node
        return rep

    monkeypatch.setattr(callback_script, "reports", scripted)
    monkeypatch.setitem(callback_script.CONFIGS, "node_off_pace", dict(callback_script.CONFIGS["print2_log_stop"],
                                                                       warn_if_node_off_pace=True, node_groups="block:4"))
    got = callback_script.drive(StragglerDetectionCallback, nvrx_straggler, make_report,
                                ("node_off_pace", "node_off_pace", 8, 0, False, False, False))
    assert got["initialize_calls"] == [dict(scores_to_compute=["relative_perf_scores", "individual_perf_scores"],
                                            gather_on_rank0=True, profiling_interval=1, report_time_interval=1.0,
                                            node_scores=True, node_groups="block:4")]
    its = got["iterations"]
    warnings = [[m for level, m in it["records"] if level == "WARNING"] for it in its]
    assert [len(w) for w in warnings] == [0, 1, 0, 0, 0, 1]  # one warning per report that names a node; a lone rank names none
    assert warnings[1] == ["STRAGGLER DETECTION WARNING: Some nodes are a little slower in nearly all of their kernels on most of "
                           "their GPUs (host fault: cooling, power, host CPU?): node node1 (pace 0.961, slower in 120 of 120 "
                           "kernels, 4 of 4 GPUs off pace)"]
    assert [it["should_stop"] for it in its] == [False] * len(sequence) and all(it["exit"] is None for it in its)  # stop_if_detected=True

    # the default, given or not: the initialize call and the transcript of today
    monkeypatch.undo()
    monkeypatch.setitem(callback_script.CONFIGS, "explicit_off", dict(callback_script.CONFIGS["print2_log_stop"],
                                                                      warn_if_node_off_pace=False))
    plain = callback_script.drive(StragglerDetectionCallback, nvrx_straggler, Report, callback_script.SCENARIOS[0])
    given = callback_script.drive(StragglerDetectionCallback, nvrx_straggler, Report,
                                  ("rank0_8ranks", "explicit_off", 8, 0, False, False, False))
    assert json.dumps(dict(given, config=None), sort_keys=True) == json.dumps(dict(plain, config=None), sort_keys=True)
    assert given["initialize_calls"] == [dict(scores_to_compute=["relative_perf_scores", "individual_perf_scores"],
                                              gather_on_rank0=True, profiling_interval=1, report_time_interval=1.0)]
    with pytest.raises(ValueError, match="warn_if_node_off_pace needs calc_relative_gpu_perf"):
        StragglerDetectionCallback(**dict(callback_script.CONFIGS["print2_log_stop"], calc_relative_gpu_perf=False,
                                          warn_if_node_off_pace=True))


# ---- 9. header, bindings and macro agree ----------------------------------------------------------------------------------------
def test_bindings_follow_the_header():
    import os
    import re

    from nvrx_straggler import _native

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nvrx_straggler.h")).read()
    symbols = {name: args for name, _, args in _native.SYMBOLS}
    for name in ("nvrx_node_score", "nvrx_report_node"):
        m = re.search(r"int " + name + r"\(([^;]*)\);", header)
        assert m, name
        assert len(m.group(1).split(",")) == len(symbols[name]), name
    m = re.search(r"#define NVRX_NODE_WORDS\(G, n_ranks, K, S\) \\\n\s*\((.*)\)\n", header)
    assert m, "NVRX_NODE_WORDS"
    expr = m.group(1).replace("(size_t)", "")
    for G, n, K, S in ((3, 5, 7, 2), (1, 1, 0, 0), (64, 64, 17, 33), (128, 1024, 128, 0)):
        assert eval(expr, {"G": G, "n_ranks": n, "K": K, "S": S}) == _native.node_words(G, n, K, S)
    assert _native.node_words(3, 5, 7, 2) == 4 * 3 * 9 + 4 * 9 + 16 * 3 + 16 * 5
    assert re.search(r"#define NVRX_ABI_VERSION 2\b", header)
    assert math.isnan(np.uint32(NAN_BITS).view(np.float32))
