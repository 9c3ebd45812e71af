"""All four row families (tail, onset, period, episode scores; nvrx_straggler/row_families.py) in ONE report on the HIP engine,
against the CPU oracle backends on the same window: tests/row_family_script.py -- two folded ranks, 64-deep rings, three rows,
a step, a beat and a stretch planted on rank 1, one ring wrapped.  Planes and scores are held to the criteria of
tests/test_gpu_{tail,onset,period,episode}.py: counts and positions exact, means within one ulp, strengths within one f32 ulp
below 1, the effective plane the oracle's function of the engine's own planes, section scores bit-exact."""
import collections

import numpy as np
import pytest

import row_family_script as script
from episode_oracle_backend import EpisodeOracleBackend, episode_excess
from onset_oracle_backend import onset_shift
from period_oracle_backend import period_excess
from tail_oracle_backend import tail_scores_table

pytestmark = pytest.mark.gpu

# per family: the planes behind plane 0, which of them are counts / positions (exact), and plane 0 as the oracle derives it
PLANES = {
    "tail": ((), (), None),
    "onset": (("before", "after", "strength", "ago", "n"), ("ago", "n"),
              lambda p: onset_shift(p["before"], p["after"], p["strength"], 0.5)),
    "period": (("peak", "rest", "strength", "period", "ago", "n"), ("period", "ago", "n"),
               lambda p: period_excess(p["period"], p["peak"], p["rest"], p["strength"], 0.5)),
    "episode": (("inside", "outside", "strength", "length", "ago", "n"), ("length", "ago", "n"),
                lambda p: episode_excess(p["length"], p["inside"], p["outside"], p["strength"], 0.5)),
}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _handles(rep):
    """``{family: (planes [ranks, P, K+S], scores [ranks, 1 + S])}`` of an unread report (the handles' own copy-out)."""
    from nvrx_straggler import row_families

    out = {}
    for fam in row_families.FAMILIES:
        planes, scores = rep.__dict__[fam.slot].handle.records()
        out[fam.name] = (np.asarray(planes, dtype=np.float32).reshape(script.LOCAL_RANKS, fam.planes, -1), np.asarray(scores))
    return out


def _two_windows(be):
    """Two reports on one workspace, the first not read before the second was issued: ``(generator, rings, [reports])``."""
    gen, rings, rows = script.make(be)
    return gen, rings, [script.report(gen, rings, rows, window=w) for w in (0, 1)]


@pytest.fixture(scope="module")
def oracle():
    """The reference, computed once: both windows on the CPU oracle -- per window the families' planes and scores, the exchange
    table they were scored with, and who was flagged."""
    from nvrx_straggler import backend

    before, cpu = backend._backend, EpisodeOracleBackend()
    backend.set_backend(cpu)
    try:
        gen, rings, rows = script.make(cpu)
        out = []
        for w in (0, 1):
            rep = script.report(gen, rings, rows, window=w)
            out.append({"handles": _handles(rep), "table": gen._ring_plan.ws.send.numpy().copy(),
                        "flagged": {fam: getattr(rep, f"identify_{fam}_stragglers")() for fam in PLANES}})
        return out
    finally:
        backend.set_backend(before)


@pytest.fixture(scope="module")
def be():
    from nvrx_straggler.backend import get_backend

    return get_backend()


def _check_family(name, got, want, table, where):
    (planes, scores), (want_planes, want_scores) = got, want
    names, exact, effective = PLANES[name]
    assert planes.shape == want_planes.shape and scores.shape == want_scores.shape == (script.LOCAL_RANKS, 1 + len(script.ROWS)), where
    if not names:
        assert np.array_equal(_bits(planes), _bits(want_planes)), (where, planes, want_planes)  # tails are samples: bit-exact
    for r in range(planes.shape[0]):
        for col in range(planes.shape[2] if names else 0):
            g = dict(zip(names, planes[r, 1:, col]))
            w = dict(zip(names, want_planes[r, 1:, col]))
            for key in names:
                if key in exact:
                    assert g[key] == w[key], (where, r, col, key, g, w)
                elif key == "strength":
                    assert abs(float(g[key]) - float(w[key])) <= 1.2e-7, (where, r, col, g, w)
                else:
                    assert abs(float(g[key]) - float(w[key])) <= float(np.spacing(w[key])), (where, r, col, key, g, w)
            assert _bits(planes[r, 0, col]) == _bits(effective(g)), (where, r, col, planes[r, :, col], g)
    exp = tail_scores_table(np.ascontiguousarray(planes[:, 0, :]), table, 0, len(script.ROWS))
    assert np.array_equal(np.isnan(scores), np.isnan(exp)), (where, scores, exp)
    ok = ~np.isnan(exp[:, 1:])
    assert np.array_equal(_bits(scores[:, 1:][ok]), _bits(exp[:, 1:][ok])), (where, scores, exp)  # one f64 quotient rounded to f32
    gpu_ok = np.isfinite(exp[:, 0])
    if gpu_ok.any():
        assert np.abs(scores[gpu_ok, 0].astype(np.float64) - exp[gpu_ok, 0].astype(np.float64)).max() <= 2e-6, where


def test_all_four_families_in_one_report_match_the_oracle_and_copy_out_once(be, oracle):
    copies = collections.Counter()
    inner = be.family_copy_out

    def counted(handle):
        copies[handle.family.name] += 1
        return inner(handle)

    be.family_copy_out = counted
    gen, rings, reports = None, None, ()
    try:
        gen, rings, reports = _two_windows(be)
        first, second = reports
        # the second report settled what the first had left on the workspace: one copy-out per family, the second's none
        assert copies == {fam: 1 for fam in PLANES}, copies
        got = [_handles(first)]
        read = {fam: getattr(first, fam + "_scores")() for fam in PLANES}
        assert copies == {fam: 1 for fam in PLANES}, copies  # reading the first report copies nothing again
        got.append(_handles(second))
        for w, rep in enumerate(reports):
            for fam in PLANES:
                _check_family(fam, got[w][fam], oracle[w]["handles"][fam], oracle[w]["table"], (w, fam))
                assert getattr(rep, f"identify_{fam}_stragglers")() == oracle[w]["flagged"][fam], (w, fam)
                per = getattr(rep, fam + "_scores")()["section_relative"]
                for row in script.ROWS:  # decisive on the engine as on the oracle
                    assert (per[row][1] < 0.75) == (script.MEANT_FOR.get(fam) == row) and per[row][0] == 1.0, (w, fam, row, per)
        assert copies == {fam: 2 for fam in PLANES}, copies
        assert read["onset"]["section_onsets"]["step"][1]["samples_ago"] == 16  # (the wrapped ring, in time order)
        assert read["tail"]["section_tails"]["beat"][0] == script.FLAT and second.tail_scores()["section_tails"]["beat"][0] == 2 * script.FLAT
    finally:
        be.family_copy_out = inner
        if gen is not None:
            gen.close()
            rings.close()


def test_period_local_before_onset_enable_raises_alike_on_both_routes(be):
    raised = []
    for backend in (be, EpisodeOracleBackend()):
        rings = backend.make_rings(1, 4, 64)
        try:
            with pytest.raises(Exception) as err:
                rings.period_local(backend.workspace(1, 0, 4, 1, 4), 64, 0.5)
            raised.append((type(err.value), str(err.value)))
        finally:
            rings.close()
    assert raised[0] == raised[1] and "onset_enable" in raised[0][1], raised
