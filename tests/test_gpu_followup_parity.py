"""GPU parity of the follow-up scorers on inputs whose relative references are alive (tests/followup_cases.py; the CPU side
of the bargain is tests/test_followup_cases_host.py): ``k_attribute`` with the column minima of its call path against
``attribute_table``, and ``k_tail_score`` behind the four row families against ``tail_scores_table`` and its siblings.  Every
record and every row of every case is compared.

Bounds, all the project's own for the same arithmetic (tests/test_gpu_attribution.py, tests/test_gpu_tail.py): kernel ids
and eligible counts exact; ``score`` / ``lost_us`` and the section slots bit for bit (one f64 quotient, or product, rounded
to f32), NaN by NaN-ness, infinities by sign; share / deficit / explained within 2e-6 absolute, W within 1e-6 relative; the
GPU slot of a family score within 2e-6 absolute (values in [0, 1]; f64 sums in another order)."""
import numpy as np
import pytest
import torch

from attribution_oracle_backend import attribute_table
from followup_cases import (FOLLOWUP_SHAPES, PLANE_KINDS, TABLE_KINDS, family_scores_table, followup_planes,
                            followup_table)
from nvrx_straggler.row_families import FAMILIES
from score_cases import COMBOS
from test_gpu_attribution import _compare as _compare_attribution
from test_gpu_attribution import _upload

pytestmark = pytest.mark.gpu

# what the module compared, printed by every case: records / rows, and how many of them had a live relative reference
_SEEN = {"attribution records": 0, "attribution records, live": 0, "attribution records, live, R >= 64": 0,
         "family rows": 0, "family rows, live GPU slot": 0, "family rows, live GPU slot, R >= 64": 0}


@pytest.fixture(scope="module")
def be():
    from nvrx_straggler.backend import get_backend

    return get_backend()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _without(exp, fam):
    """``exp`` with family ``fam`` not computed: what ``attribute_table`` writes for it."""
    out = exp.copy()
    out.view(np.float32)[:, fam, :, :] = np.float32(np.nan)
    out.view(np.int32)[:, fam, 1:, 0] = -1
    out[:, fam, 0, 2] = 0
    out.view(np.float32)[:, fam, 0, 3] = 0.0
    return out


@pytest.mark.parametrize("R,K,S", FOLLOWUP_SHAPES)
@pytest.mark.parametrize("kind", TABLE_KINDS)
def test_attribution_matches_the_formula(be, kind, R, K, S):
    T = followup_table(kind, R, K, S)
    ws = _upload(be, T, K, S)
    full = {}
    for n in (1, 5, 16):
        both = attribute_table(T, K, S, n, True, True)
        for do_indiv, do_rel in COMBOS:
            got = be.attribute(ws, ws.send, n, do_indiv, do_rel).records()
            exp = both if do_indiv and do_rel else _without(both, 0 if not do_indiv else 1)
            _compare_attribution(got, exp, (kind, R, K, S, do_indiv, do_rel, n), edge_values=True)
            full[(do_indiv, do_rel, n)] = got
            live = int((exp[:, 1, 0, 2] > 0).sum())
            _SEEN["attribution records"] += 2 * R
            _SEEN["attribution records, live"] += live
            _SEEN["attribution records, live, R >= 64"] += live if R >= 64 else 0
    if kind != "edge" and K >= 2:  # (an "edge" table's kernel-less rank leaves the relative family empty, by design)
        assert (full[(True, True, 16)][:, 1, 0, 2] > 0).all()
    # a sub-range of ranks is the slice of the full result, word for word
    lo = R // 3
    n_ranks = max(1, min(R - lo, 5))
    for n in (5, 16):
        part = be.attribute(ws, ws.send, n, True, True, first_rank=lo, n_ranks=n_ranks).records()
        assert np.array_equal(part, full[(True, True, n)][lo : lo + n_ranks]), (kind, R, K, S, n)
    print(_SEEN)


def _family_score(be, fam, planes, T, K, S, first_rank=0, n_ranks=None):
    R = T.shape[0]
    ws = be.workspace(R, K, S, R, 0)
    ws.family_settle(fam)
    ws.send.copy_(torch.from_numpy(T))
    _, table, _, _ = ws.family_buffers(fam)
    if table.numel():
        table.copy_(torch.from_numpy(planes.reshape(R, -1)))
    torch.cuda.synchronize()
    handle = be._family_score(fam, ws, table, ws.send, first_rank, n_ranks, (950000,) if fam.name == "tail" else ())
    got_planes, scores = handle.records()
    hi = R if n_ranks is None else first_rank + n_ranks
    # the planes handed back are the input, bit for bit, all P of them
    assert np.array_equal(_bits(got_planes).reshape(hi - first_rank, fam.planes, K + S), _bits(planes[first_rank:hi]))
    return scores


def _compare_family(got, exp, tag):
    R, S = exp.shape[0], exp.shape[1] - 1
    assert got.shape == exp.shape and got.dtype == exp.dtype == np.float32, tag
    assert np.array_equal(np.isnan(got), np.isnan(exp)), (tag, "NaN", np.argwhere(np.isnan(got) != np.isnan(exp))[:8])
    assert np.array_equal(np.isposinf(got), np.isposinf(exp)) and np.array_equal(np.isneginf(got), np.isneginf(exp)), (tag, "inf")
    sec_ok = ~np.isnan(exp[:, 1:])
    bad = np.argwhere(sec_ok & (_bits(got[:, 1:]) != _bits(exp[:, 1:])))
    assert bad.size == 0, (tag, "sections", bad[:8].tolist())  # one f64 quotient rounded to f32
    fin = np.isfinite(exp[:, 0])
    if fin.any():
        err = np.abs(got[fin, 0].astype(np.float64) - exp[fin, 0].astype(np.float64)).max()
        assert err <= 2e-6, (tag, "GPU slot", err)
    return int(fin.sum())


@pytest.mark.parametrize("R,K,S", FOLLOWUP_SHAPES)
@pytest.mark.parametrize("kind", PLANE_KINDS)
@pytest.mark.parametrize("fam", FAMILIES, ids=lambda f: f.name)
def test_family_score_matches_numpy(be, fam, kind, R, K, S):
    planes, T = followup_planes(kind, fam, R, K, S)
    got = _family_score(be, fam, planes, T, K, S)
    exp = family_scores_table(fam, planes, T, K, S)
    assert got.shape == exp.shape == (R, 1 + S)
    live = _compare_family(got, exp, (fam.name, kind, R, K, S))
    if K >= 2 and R >= 2:
        assert live >= R - 3  # every rank but the two without weights and the one with the 0/0 kernel column
    _SEEN["family rows"] += R
    _SEEN["family rows, live GPU slot"] += live
    _SEEN["family rows, live GPU slot, R >= 64"] += live if R >= 64 else 0
    # a sub-range of ranks equals the slice of the full result
    lo, n = (R // 3, max(1, R // 2)) if R > 1 else (0, 1)
    part = _family_score(be, fam, planes, T, K, S, lo, n)
    assert np.array_equal(_bits(part), _bits(got[lo : lo + n]))
    print(_SEEN)
