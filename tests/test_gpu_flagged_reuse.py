"""The flagged sets of a resident report in the benchmark's pattern (``rep, found = step()``, the previous ``found`` dropped by
rebinding): ``_nvrx_pyread.flagged`` hands dropped results out again, and every one of them must still be what the general
decode of the same report says, in objects of its own."""
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu


def test_flagged_sets_of_fifty_reports_in_the_benchmark_pattern(monkeypatch):
    from nvrx_straggler import reporting
    from nvrx_straggler.folded import FoldedJob

    R, S, n, slow = 2, 4, 64, 1
    names = [synth.section_name(s) for s in range(S)]
    job = FoldedJob(total_ranks=R, section_names=names, ring_cap=n, node_name="n")
    try:
        for lr, r in enumerate(job.logical_ranks()):
            job.load(lr, synth.stress_samples(r, S, n, slow_rank=slow, slow_factor=1.5))
        torch.cuda.synchronize()

        def step():
            job.rearm(n)
            rep = job.report()
            return rep, rep.identify_stragglers()

        def objects_of(found):
            out = list(found.values())
            for k in ("straggler_sections_relative", "straggler_sections_individual"):
                out.extend(found[k].values())
            return out

        fast_reads = []
        decode = reporting._ScoreSource.flagged

        def counted(self, rank_to_node, thresholds):
            out = decode(self, rank_to_node, thresholds)
            fast_reads.append(out is not None)
            return out

        monkeypatch.setattr(reporting._ScoreSource, "flagged", counted)
        rep = found = None
        for i in range(50):
            before = None if found is None else (found, objects_of(found))
            rep, found = step()
            with monkeypatch.context() as m:
                m.setattr(reporting._ScoreSource, "flagged", lambda self, a, b: None)
                want = rep.identify_stragglers()
            assert found == want, i
            for k in ("straggler_sections_relative", "straggler_sections_individual"):
                assert list(found[k]) == list(want[k]) and all(type(v) is set for v in found[k].values())
            assert {x.rank for x in found["straggler_gpus_relative"]} <= {slow}
            assert {k: {x.rank for x in v} for k, v in found["straggler_sections_relative"].items()} == {name: {slow} for name in names}
            if before is not None:  # the previous result is still alive here: nothing of it is in this one
                assert found is not before[0]
                mine = {id(o) for o in objects_of(found)}
                assert len(mine) == len(objects_of(found)) and not mine & {id(o) for o in before[1]}
        assert sum(fast_reads) >= 40  # (planned reports are read by the C decoder: that is the path under test)
    finally:
        job.close()
