"""The one path robust, peer, pace-per-group and node scores share (nvrx_straggler/table_families.py), on the GPU, with all four
on at once: four families in flight on one workspace, pace and pace-per-group in one slot, and one ``settle_readers`` that
delivers all of them.  Every family's records are compared with the restatement, and by the comparison, of its own test."""
import numpy as np
import pytest
import torch

from node_oracle_backend import node_scores_table
from pace_group_oracle_backend import pace_group_scores_table
from peer_oracle_backend import peer_scores_table
from robust_oracle_backend import robust_scores_table
from test_gpu_node import _compare as _compare_node
from test_gpu_pace_group import _compare as _compare_pace_group
from test_gpu_peer import _compare as _compare_peer
from test_gpu_robust import _compare as _compare_robust

pytestmark = pytest.mark.gpu

R, K, S, SAMPLES = 8, 5, 2, 16
IN_FLIGHT = ["robust", "peer", "pace_group", "node"]  # in the order settle_readers delivers them


def test_four_families_of_one_asynchronous_report_are_delivered_by_the_next_and_copied_out_once():
    from nvrx_straggler.backend import get_backend
    from nvrx_straggler.folded import FoldedJob
    from nvrx_straggler.table_families import FAMILIES

    torch.cuda.set_device(0)
    be = get_backend()
    calls = []  # (family, handle, records) of every copy-out, in the order they ran

    def counted(name, inner):
        def copy_out(handle):
            records = inner(handle)
            calls.append((name, handle, records))
            return records

        return copy_out

    for fam in FAMILIES:
        setattr(be, fam.name + "_copy_out", counted(fam.name, getattr(be, fam.name + "_copy_out")))
    job = FoldedJob(total_ranks=R, section_names=["fwd", "bwd"], ring_cap=64, scores_to_compute=("relative_perf_scores",),
                    kernel_names=[f"kernel_{k}" for k in range(K)], robust_scores=True, peer_groups="block:4", pace_scores=True,
                    pace_peer_groups=True, node_scores=True, node_groups="block:2", asynchronous=True)
    try:
        rng = np.random.default_rng(2026)
        reports, tables, by_issue = [], [], []
        for i in range(3):  # the general report, then two planned ones on one workspace
            for lr in range(R):
                job.load(lr, rng.lognormal(np.log(1000.0 * (i + 1)), 0.2, (S, SAMPLES)).astype(np.float32))
                job.load_kernels(lr, rng.lognormal(np.log(100.0 * (i + 1)), 0.2, (K, SAMPLES)).astype(np.float32))
            before = len(calls)
            reports.append(job.report())  # (nothing of it is read before the next one is issued)
            by_issue.append(calls[before:])
            plan = job.reporter._ring_plan
            assert plan is not None and (i == 0 or job.reporter._last_plan_fused is True)
            ws = plan.ws
            assert (ws.R, ws.K, ws.S) == (R, K, S)
            be.synchronize()
            torch.cuda.synchronize()
            tables.append(ws.table.cpu().numpy().copy())
        # issuing the third report delivered the second's four families: one copy-out each, in settle_readers' order
        assert [name for name, _, _ in by_issue[2]] == IN_FLIGHT, [name for name, _, _ in by_issue[2]]
        assert all(st.last is not None for st in ws._table_state.values()) and sorted(ws._table_state) == ["node", "pace", "peer", "robust"]
        first, second, last = reports
        assert first.robust_scores() and first.peer_scores() and first.pace_scores() and first.node_scores()  # (the general one)
        n = len(calls)
        assert second.robust_scores() and second.peer_scores() and second.pace_scores() and second.node_scores()
        assert len(calls) == n  # the second was delivered already: reading it copies nothing
        assert last.robust_scores() and last.peer_scores() and last.pace_scores() and last.node_scores()
        assert sorted(name for name, _, _ in calls[n:]) == sorted(IN_FLIGHT)  # the third's, on first read ...
        assert last.robust_scores() and last.node_scores() and len(calls) == n + 4  # ... and once
        names = [name for name, _, _ in calls]
        assert {name: names.count(name) for name in IN_FLIGHT} == dict.fromkeys(IN_FLIGHT, 3) and "pace" not in names
        assert len({id(h) for _, h, _ in calls}) == len(calls)  # one copy-out per handle

        peers, nodes = job.reporter._peer_for(ws), job.reporter._node_for(ws)
        assert (peers.G, peers.max_size, nodes.G, nodes.max_size) == (2, 4, 4, 2)
        for i, delivered in ((1, by_issue[2]), (2, calls[n:])):
            T = tables[i]
            for name, h, got in delivered:
                tag = ("report", i, name)
                assert (h.first_rank, h.n_ranks, h.K, h.S) == (0, R, K, S) and h.family.name == name, tag
                if name == "robust":
                    assert h.G == 0
                    _compare_robust(got, robust_scores_table(T, K, S, 0, R, h.min_ranks, h.floor_rel), tag)
                elif name == "peer":
                    assert h.G == peers.G
                    _compare_peer(got, peer_scores_table(T, K, S, peers.host, peers.G, 0, R, h.min_ranks), tag)
                elif name == "pace_group":
                    assert h.G == peers.G
                    _compare_pace_group(got, pace_group_scores_table(T, K, S, peers.host, peers.G, peers.max_size, 0, R, h.min_ranks,
                                                                     h.min_peers), tag)
                else:
                    assert h.G == nodes.G
                    _compare_node(got, node_scores_table(T, K, S, nodes.host, nodes.G, nodes.max_size, h.min_members, h.min_nodes,
                                                         0, R), tag)
        assert not np.array_equal(tables[1], tables[2])  # (two windows that differ: neither report could pass for the other)
    finally:
        job.close()
        for fam in FAMILIES:
            del be.__dict__[fam.name + "_copy_out"]
