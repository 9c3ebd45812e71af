"""``_nvrx_pyread.flagged`` on a memo hit: a result the caller has dropped is handed out again instead of a copy
(csrc/nvrx_pyread.c, "handing a dropped flagged result out again").  CPU only; every answer is compared with the general
decode (``_DeviceFlags.decode``), whatever the caller did to the results it was given before."""
import gc
import platform
import sys
import weakref

import numpy as np
import pytest

from nvrx_straggler import reporting

pr = reporting._pyread
assert pr is not None and hasattr(pr, "flagged"), "csrc/nvrx_pyread.c is not built"

# where the extension reuses at all (elsewhere every hit is a copy, and only the equalities below apply)
REUSES = platform.python_implementation() == "CPython" and sys.version_info < (3, 14) and getattr(sys, "_is_gil_enabled", lambda: True)()

SHAPES = [(R, S, with_cols) for R in (2, 8) for S in (1, 3, 64) for with_cols in (False, True)]
PARTS = ("gpu_rel", "gpu_indiv", "sec_rel", "sec_indiv")


class Case:
    """One view's arguments of ``flagged`` and the general decode of a flag table."""

    def __init__(self, R, S, with_cols, kind="slow_rank", seed=0):
        self.R, self.S, self.W = R, S, 2 + 2 * S
        rng = np.random.default_rng(seed + 1000 * R + S)
        self.ids = [reporting.StragglerId(rank=r, node=f"node{r // 4}") for r in range(R)]
        self.names = tuple(f"section_{i:02d}" for i in range(S))
        self.cols = tuple(int(c) for c in rng.permutation(S)) if with_cols else None
        self.memo = [None, None, None, None]
        self.set_table(kind, rng)

    def set_table(self, kind, rng=None):
        flags = np.zeros((self.R, self.W), dtype=np.uint8)
        if kind == "slow_rank":  # one rank flagged in everything, as the benchmark's rank 3
            flags[self.R - 1, :] = 1
        elif kind == "other_rank":
            flags[0, :] = 1
        elif kind == "random":  # several members per set, some columns without any
            flags[:] = rng.random((self.R, self.W)) < 0.4
            flags[0, 2] = flags[0, 2 + self.S] = 1  # (each of the two dicts has a key at every size)
        self.flags = flags
        self.buf = flags.tobytes()
        cols = {n: (self.cols[i] if self.cols is not None else i) for i, n in enumerate(self.names)}
        dec = reporting._DeviceFlags((0.75,) * 4, flags, range(self.R), list(self.names), cols, self.S, True, True)
        self.want = dec.decode(self.ids)

    def call(self, memo=None, has_rel=True, has_indiv=True):
        return pr.flagged(self.buf, 0, self.R, self.W, self.S, has_rel, has_indiv, self.ids, self.names, self.cols,
                          self.memo if memo is None else memo)

    def check(self, got, want=None):
        want = self.want if want is None else want
        assert type(got) is tuple and len(got) == 4
        for part, g, w in zip(PARTS, got, want):
            assert g == w, part
        assert type(got[0]) is set and type(got[1]) is set
        for g, w in zip(got[2:], want[2:]):
            assert type(g) is dict and list(g) == list(w)
            assert all(type(v) is set for v in g.values())
        return got


def objects_of(result):
    out = list(result)
    for d in result[2:]:
        out.extend(d.values())
    return out


@pytest.mark.parametrize("kind", ["slow_rank", "random"])
@pytest.mark.parametrize("R,S,with_cols", SHAPES)
def test_every_result_equals_the_general_decode(R, S, with_cols, kind):
    c = Case(R, S, with_cols, kind)
    c.check(c.call())                       # the miss
    for _ in range(6):                      # hits, each result dropped at once
        c.check(c.call())
    found = None
    for _ in range(6):                      # the benchmark's pattern: the previous result dies after the next call
        found = c.check(c.call())
    held = [c.check(c.call()) for _ in range(4)]   # every result held
    for r in held:
        c.check(r)
    c.check(found)


@pytest.mark.parametrize("R,S,with_cols", SHAPES)
def test_two_results_alive_at_once_share_nothing(R, S, with_cols):
    c = Case(R, S, with_cols, "random")
    a = c.call()
    b = c.call()
    d = c.call()
    for x, y in ((a, b), (b, d), (a, d)):
        ids_x = {id(o) for o in objects_of(x)}
        assert len(ids_x) == len(objects_of(x))
        assert not ids_x & {id(o) for o in objects_of(y)}
    a[2].clear(), a[0].add("mine")
    c.check(b), c.check(d)


@pytest.mark.skipif(not REUSES, reason="this interpreter always copies")
@pytest.mark.parametrize("R,S,with_cols", SHAPES)
def test_a_dropped_result_is_handed_out_again(R, S, with_cols):
    """The point of it all: in the benchmark's pattern call N returns the objects of call N - 2."""
    c = Case(R, S, with_cols, "random")
    found = c.call()
    seen = []
    for _ in range(6):
        found = c.check(c.call())
        seen.append([id(o) for o in objects_of(found)])
    assert seen[2] == seen[4] and seen[3] == seen[5] and seen[4] != seen[5]
    del found
    x, y, z = ([id(o) for o in objects_of(c.check(c.call()))] for _ in range(3))   # dropped at once: the two kept results in turn
    assert x == z and x != y and {tuple(x), tuple(y)} == {tuple(seen[4]), tuple(seen[5])}


def _add_member(r, c):
    r[2][next(iter(r[2]))].add(reporting.StragglerId(rank=99, node="x"))


def _remove_member(r, c):
    r[3][next(iter(r[3]))].pop()


def _clear_set(r, c):
    r[2][next(iter(r[2]))].clear()


def _clear_gpu_set(r, c):
    r[0].clear()


def _delete_key(r, c):
    del r[2][next(iter(r[2]))]


def _add_key(r, c):
    r[3]["not a section"] = {c.ids[0]}


def _reorder(r, c):
    k = next(iter(r[2]))
    r[2][k] = r[2].pop(k)


def _frozenset_value(r, c):
    k = next(iter(r[2]))
    r[2][k] = frozenset(r[2][k])


def _list_value(r, c):
    k = next(iter(r[3]))
    r[3][k] = list(r[3][k])


def _swap_values(r, c):
    ks = list(r[2])
    a, b = ks[0], ks[-1]
    r[2][a], r[2][b] = r[2][b], r[2][a]


def _same_size_other_member(r, c):
    s = r[2][next(iter(r[2]))]
    s.pop()
    s.add(reporting.StragglerId(rank=99, node="x"))


def _remove_and_put_back(r, c):  # equal again, but its table now has a deleted entry
    s = r[2][next(iter(r[2]))]
    m = s.pop()
    s.add(m)


def _grow_and_shrink(r, c):  # equal again, in a table that has been resized
    s = r[3][next(iter(r[3]))]
    extra = [reporting.StragglerId(rank=100 + i, node="x") for i in range(40)]
    s.update(extra)
    s.difference_update(extra)


MUTATIONS = [_add_member, _remove_member, _clear_set, _clear_gpu_set, _delete_key, _add_key, _reorder, _frozenset_value, _list_value,
             _swap_values, _same_size_other_member, _remove_and_put_back, _grow_and_shrink]


@pytest.mark.parametrize("mutate", MUTATIONS, ids=lambda f: f.__name__.lstrip("_"))
@pytest.mark.parametrize("kind", ["slow_rank", "random"])
@pytest.mark.parametrize("R,S,with_cols", SHAPES)
def test_a_mutated_result_never_comes_back(R, S, with_cols, kind, mutate):
    c = Case(R, S, with_cols, kind)
    c.call()
    for held_too in (False, True):           # the mutated result in either of the memo's two places
        r = c.check(c.call())
        other = c.check(c.call()) if held_too else None
        mutate(r, c)
        del r
        a = c.check(c.call())
        b = c.check(c.call())
        c.check(a)
        del a, b, other
        c.check(c.call())


@pytest.mark.parametrize("R,S,with_cols", SHAPES)
def test_what_the_caller_keeps_is_left_alone(R, S, with_cols):
    c = Case(R, S, with_cols, "random")
    c.call()
    # one inner set kept, the rest dropped
    r = c.call()
    name = next(iter(r[2]))
    mine = r[2][name]
    before = set(mine)
    del r
    later = [c.check(c.call()) for _ in range(3)]
    later.append(c.check(c.call()))
    for res in later:
        assert all(o is not mine for o in objects_of(res))
    assert mine == before
    # only sec_rel kept
    sr = c.call()[2]
    snapshot = {k: set(v) for k, v in sr.items()}
    kept = [sr] + list(sr.values())
    for _ in range(4):
        res = c.check(c.call())
        assert all(o is not k for o in objects_of(res) for k in kept)
    assert sr == snapshot and list(sr) == list(snapshot)
    # the result tuple itself kept: nothing of it is handed out
    t = c.call()
    kept = objects_of(t)
    for _ in range(4):
        res = c.check(c.call())
        assert res is not t and all(o is not k for o in objects_of(res) for k in kept)
    c.check(t)


def test_a_weak_reference_to_an_inner_set_blocks_reuse():
    c = Case(8, 64, False, "slow_rank")
    c.call()
    r = c.call()
    inner = r[2][c.names[5]]
    ref = weakref.ref(inner)
    marks = [id(o) for o in objects_of(r)]
    del r, inner
    if REUSES:
        assert ref() is not None            # the memo still holds the result ...
    for _ in range(2):                      # ... and never hands it out
        res = c.check(c.call())
        assert all(o is not ref() for o in objects_of(res))
        if ref() is not None:
            assert [id(o) for o in objects_of(res)] != marks
    for _ in range(3):
        found = c.check(c.call())           # noqa: F841  (held across the next call)
    gc.collect()
    assert ref() is None                    # pushed out of the memo: gone


def test_results_follow_the_flag_bytes():
    c = Case(8, 64, True, "slow_rank")
    rng = np.random.default_rng(5)
    wants = {}
    for kind in ("slow_rank", "other_rank", "slow_rank", "random", "none", "slow_rank", "slow_rank", "other_rank"):
        c.set_table(kind, rng)
        wants.setdefault(kind, c.want)
        found = None
        for _ in range(3):
            found = c.check(c.call())       # noqa: F841
    assert wants["none"] == (set(), set(), {}, {})


def test_a_memo_shared_across_views_misses():
    a, b = Case(8, 3, False, "slow_rank"), Case(8, 3, True, "slow_rank")
    b.ids, b.names = a.ids, a.names
    b.set_table("slow_rank")
    other_names = Case(8, 3, False, "slow_rank")
    other_names.ids, other_names.names = a.ids, ("x", "y", "z")
    other_names.set_table("slow_rank")
    memo = [None, None, None, None]
    for _ in range(3):
        for c in (a, b, other_names):
            found = c.check(c.call(memo))   # noqa: F841
            rel_only = c.call(memo, has_indiv=False)
            assert rel_only[1] == set() and rel_only[3] == {} and rel_only[0] == c.want[0] and rel_only[2] == c.want[2]
            indiv_only = c.call(memo, has_rel=False)
            assert indiv_only[0] == set() and indiv_only[2] == {} and indiv_only[1] == c.want[1] and indiv_only[3] == c.want[3]
    # a memo without the two places for results (the earlier shape) still works: every hit a copy
    short = [None, None]
    x, y = a.check(a.call(short)), a.check(a.call(short))
    assert not {id(o) for o in objects_of(x)} & {id(o) for o in objects_of(y)} and len(short) == 2
    with pytest.raises(ValueError):
        a.call([None, None, None])


def test_nothing_leaks():
    c = Case(8, 64, False, "slow_rank")
    tracked = c.ids + list(c.names)
    found = c.call()
    found = c.call()
    held = [c.call() for _ in range(8)]
    del held[:]
    gc.collect()
    refs = [sys.getrefcount(o) for o in tracked]
    blocks = sys.getallocatedblocks()
    for _ in range(20000):
        found = c.call()
    held = []
    for _ in range(20000):
        held.append(c.call())
    c.check(held[0]), c.check(held[-1])
    del held[:]
    gc.collect()
    assert abs(sys.getallocatedblocks() - blocks) < 64, (sys.getallocatedblocks(), blocks)
    c.check(found)
    assert [sys.getrefcount(o) for o in tracked] == refs
