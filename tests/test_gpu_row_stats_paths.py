"""Every selection path of the statistics kernel, in every launch shape ``pick_variant`` can return, shown to have run.

Per launch shape, at its smallest and its largest stride, the recipes of tests/row_stats_cases.py go through ``be.row_stats``
for both kinds and for counts of stride, stride - 1 and stride - 3.  Every row's selections are the oracle's bit for bit, its
moments are within the bounds of tests/test_gpu_row_stats.py wherever the samples span a moderate range, and word 7 of its
statistics row -- the path the kernel says it took -- is the one the model of tests/row_stats_cases.py works out from the
kernel's constants.  The cells (path, finish, placement, edge) for which the GPU agreed are printed as a census and must
contain ``REQUIRED`` for the shape, for both kinds and both parities of n."""
import numpy as np
import pytest

import row_stats_cases as rc
from oracle import oracle
from test_gpu_row_stats import _check_against_oracle, _run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    from nvrx_straggler.backend import get_backend

    return get_backend()


@pytest.mark.parametrize("shape", tuple(rc.REACHABLE), ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_selection_path_runs_in_this_launch_shape(be, shape):
    census = {}      # (kind, parity of n) -> cell -> recipes
    paths = set()
    worst = {}       # (path word, kind) -> [worst AVG error, worst STD error] relative to the oracle, over the moderate rows
    moderate = np.array([r.moderate for r in rc.RECIPES])
    for stride in rc.REACHABLE[shape]:
        for less in rc.COUNTS:
            m, counts, plans = rc.matrix(stride, less)
            for kind in (0, 1):
                kinds = np.full(len(plans), kind, np.uint8)
                got = _run(be, m, counts, kinds)
                tag = f"<{shape[0]},{shape[1]}> stride {stride} n {stride - less} kind {kind}"
                # selections and moments against the oracle, with the bounds the random suite uses
                _check_against_oracle(got[moderate], m[moderate], counts[moderate], kinds[moderate], tag)
                exp = oracle.rows_stats(m, counts, kinds)
                for r, (rec, plan) in enumerate(zip(rc.RECIPES, plans)):
                    n = int(counts[r])
                    if not rec.moderate and n:
                        for c, name in ((0, "MIN"), (1, "MAX"), (2, "MED")):
                            # (== on the values: the signed-zero row may answer 0.0 for -0.0)
                            assert got[r, c] == np.float32(exp[r, c]), (tag, rec.name, name, got[r, c], exp[r, c])
                        assert got[r, 5] == n
                    assert got[r, 7] == plan.path, (tag, rec.name, "word 7", got[r, 7], plan)
                    for cell in rc.cells_of(plan):
                        census.setdefault((kind, n & 1), {}).setdefault(cell, set()).add(rec.name)
                    paths.add(int(got[r, 7]))
                    if rec.moderate and n > 1 and plan.path:
                        w = worst.setdefault((plan.path, kind), [0.0, 0.0])
                        w[0] = max(w[0], abs(got[r, 3] - exp[r, 3]) / abs(exp[r, 3]))
                        w[1] = max(w[1], abs(got[r, 4] - exp[r, 4]) / abs(exp[r, 4]))
    for (kind, parity), cells in sorted(census.items()):
        print(f"[census <{shape[0]},{shape[1]}> kind {kind} {'odd' if parity else 'even'} n]")
        for cell, names in sorted(cells.items(), key=lambda c: (c[0][0], str(c[0]))):
            if cell[1] is not None and (cell[2] is not None or cell[1] not in ("one_wave", "all_waves")):
                print(f"    {cell}: {', '.join(sorted(names))}")
    for (path, kind), (avg, std) in sorted(worst.items()):
        print(f"[moments <{shape[0]},{shape[1]}> path {path} kind {kind}] worst relative error: AVG {avg:.3g} STD {std:.3g}")
    for (kind, parity), cells in census.items():
        missing = rc.required(shape, parity) - set(cells)
        assert not missing, (shape, kind, parity, sorted(missing, key=str))
    assert len(census) == 4
    assert not (paths & rc.IMPOSSIBLE.get(shape, frozenset())), (shape, paths)
    # the moments of every path word have been compared with the oracle's
    assert set(worst) == {(p, kind) for p in paths - {0} for kind in (0, 1)}, (shape, worst, paths)
