"""The model of the statistics kernel's selection (tests/row_stats_cases.py) and its recipes, checked on the CPU: the model
follows a CORRECT selection (it ends on the row's lower median), ``pick`` has the boundaries of ``pick_variant``, and the
recipes reach every cell that tests/test_gpu_row_stats_paths.py requires the GPU to reach, in every launch shape."""
import numpy as np
import pytest

import row_stats_cases as rc

SHAPES = tuple(rc.REACHABLE)


def test_pick_maps_every_stride_to_a_reachable_shape_with_the_stated_boundaries():
    seen, prev = {}, None
    for stride in range(4, 65536 + 4, 4):
        shape = rc.pick(stride)
        assert shape in rc.REACHABLE, stride
        if shape != prev:
            assert shape not in seen, stride                      # one contiguous stretch of strides per shape
            seen[shape] = [stride, stride]
        seen[shape][1] = stride
        prev = shape
    assert {s: tuple(v) for s, v in seen.items()} == rc.REACHABLE
    assert len(rc.REACHABLE) == 14 and rc.pick(65540) is None
    assert rc.REACHABLE[(512, 6)] == (10244, 12288) and rc.REACHABLE[(512, 12)] == (20484, 24576)
    assert rc.REACHABLE[(1024, 12)] == (40964, 49152)
    for (threads, vpt), (lo, hi) in rc.REACHABLE.items():
        assert hi == threads * vpt * 4 and vpt in rc.VPTS


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_model_ends_on_the_lower_median_and_the_recipes_reach_every_required_cell(shape):
    threads, vpt = shape
    reached = {0: set(), 1: set()}
    paths = set()
    for stride in rc.REACHABLE[shape]:
        assert rc.pick(stride) == shape
        for less in rc.COUNTS:
            m, counts, plans = rc.matrix(stride, less)
            for rec, x, n, plan in zip(rc.RECIPES, m, counts.tolist(), plans):
                if n == 0:
                    assert plan.cls == "empty" and plan.path == 0
                else:
                    keys = rc.raw_keys(x, n)
                    assert plan.conv == bool((keys >> 31).any())
                    keys = np.sort(rc.f2key(keys) if plan.conv else keys)
                    assert plan.med_key == keys[(n - 1) >> 1], (rec.name, stride, n, plan)
                    assert (plan.cls == "equal") == (keys[0] == keys[-1])
                    assert (plan.path & 4 != 0) == (plan.refinements > 0) and plan.refinements <= 3
                    assert (plan.edge is not None) == (plan.path in (2, 6))
                    assert plan.path in (0, 1, 2, 5, 6, 18, 22)
                    if plan.cls in ("one_wave", "all_waves"):
                        assert (plan.pop <= rc.CAND_ONE) == (plan.cls == "one_wave") and plan.pop <= rc.CAND_MAX
                reached[n & 1] |= rc.cells_of(plan)
                paths.add(plan.path)
    for parity in (0, 1):
        missing = rc.required(shape, parity) - reached[parity]
        assert not missing, (shape, "odd n" if parity else "even n", sorted(missing, key=str))
    assert not (paths & rc.IMPOSSIBLE.get(shape, frozenset())), (shape, paths)


def test_the_even_rows_reach_every_way_to_the_second_middle():
    """rank k+1 equal to rank k, the next greater key in another wave than the median or in the same one, the next greater key
    being the row's maximum, n = 2: each in every launch shape (at its largest stride; the smallest stride of <256,1> is one
    float4, which has no second wave)."""
    for shape, (_, stride) in rc.REACHABLE.items():
        _, counts, plans = rc.matrix(stride, 0)
        seen = {p.second for p, n in zip(plans, counts) if n and n % 2 == 0}
        assert {"equal", "other_wave", "same_wave"} <= seen, (shape, seen)
        assert any(p.second_is_max and n > 2 for p, n in zip(plans, counts)), shape
        assert any(n == 2 for n in counts)


def test_the_tile_boundary_rows_sit_on_both_sides_of_the_speculation_switch():
    for shape, (_, stride) in rc.REACHABLE.items():
        _, counts, _ = rc.matrix(stride, 0)
        names = [r.name for r in rc.RECIPES]
        at, past = int(counts[names.index("n=tile")]), int(counts[names.index("n=tile+1")])
        assert at == min(4 * shape[0], stride) and past == min(4 * shape[0] + 1, stride)
