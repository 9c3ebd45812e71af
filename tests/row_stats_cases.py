"""Rows that steer the statistics kernel (``k_row_stats``) down every selection path, and a NumPy model of that selection's
control flow (tests/test_row_stats_cases_host.py on the CPU, tests/test_gpu_row_stats_paths.py on the GPU).

The kernel writes the path it took into word 7 of a statistics row (include/nvrx_straggler.h).  ``selection_plan`` restates
only the CONTROL FLOW of the selection -- the tile-0 range estimate, the histogram's shift, the clamping, ``locate``, the
rebuild, the re-keying, the refinement loop -- with the kernel's constants and none of its output, and says which path, which
finish and which sub-branches a row must take in a given launch shape.  A GPU test compares word 7 with it and keeps a census
of the (launch shape, cell) pairs that ran; ``REQUIRED`` is what that census has to contain."""
from typing import NamedTuple, Optional

import numpy as np

CAND_MAX = 256   # a selected bin this small is ranked directly ...
CAND_ONE = 64    # ... and one this small by a single wave
VPTS = (1, 2, 3, 4, 5, 6, 8, 10, 12, 16)

# launch shape -> (smallest, largest) row stride that selects it
REACHABLE = {
    (256, 1): (4, 1024),
    (256, 2): (1028, 2048),
    (512, 2): (2052, 4096),
    (512, 3): (4100, 6144),
    (512, 4): (6148, 8192),
    (512, 5): (8196, 10240),
    (512, 6): (10244, 12288),
    (512, 8): (12292, 16384),
    (512, 10): (16388, 20480),
    (512, 12): (20484, 24576),
    (512, 16): (24580, 32768),
    (1024, 10): (32772, 40960),
    (1024, 12): (40964, 49152),
    (1024, 16): (49156, 65536),
}


def pick(stride):
    """``pick_variant``: the preferred width (256 threads up to 2048 samples, else 512, else 1024) and the smallest register
    tile of that width that holds the row."""
    for threads in ((256, 512, 1024) if stride <= 256 * 4 * 2 else (512, 1024, 256)):
        for vpt in VPTS:
            if threads * vpt * 4 >= stride:
                return threads, vpt
    return None


def hist_bits(threads):
    return 11 if threads == 256 else 12


class Plan(NamedTuple):
    path: int                     # word 7
    cls: str                      # empty / equal / direct / one_wave / all_waves / refined_to_one_key
    refinements: int
    pop: int                      # population of the bin the selection ends in
    lane3: bool                   # some thread holds three or more members of a ranked bin
    edge: Optional[str]           # "low" / "high": the edge bin that caused a rebuild
    second: Optional[str]         # even rows: "equal", "other_wave" or "same_wave" (rank k+1 against rank k)
    second_is_max: bool           # even rows: the next greater key is the row's maximum
    med_key: Optional[int]        # the key the selection ends on
    conv: bool                    # keys are f2key(x), not the raw bits


def raw_keys(x, n):
    return np.ascontiguousarray(x[:n], dtype=np.float32).view(np.uint32).astype(np.int64)


def f2key(u):
    return np.where(u >> 31 != 0, u ^ 0xFFFFFFFF, u ^ 0x80000000)


def _locate(hist, k):
    """Bin holding rank ``k``, the rank inside it, its population."""
    c = np.cumsum(hist)
    b = int(np.searchsorted(c, k, side="right"))
    return b, k - (int(c[b - 1]) if b else 0), int(hist[b])


def _shift(span, hb):
    return max(int(span).bit_length() - hb, 0)       # 32 - clz(span), less the histogram's bits, floored at 0


def selection_plan(x, n, threads, vpt):
    hb = hist_bits(threads)
    nb = 1 << hb
    tile = 4 * threads
    if n == 0:
        return Plan(0, "empty", 0, 0, False, None, None, False, None, False)
    keys = raw_keys(x, n)
    speculative = vpt > 1 and n > tile
    mn0, mx0 = int(keys[:tile].min()), int(keys[:tile].max())
    R = mx0 - mn0 if speculative else 0
    lo0 = mn0 - R if mn0 > R else 0
    hi0 = mx0 + R if mx0 < 0xFFFFFFFF - R else 0xFFFFFFFF
    sh = _shift(hi0 - lo0, hb)
    kmn, kmx = int(keys.min()), int(keys.max())
    conv = kmx >= 0x80000000
    first = keys
    if conv:
        keys = f2key(keys)
        kmn, kmx = int(keys.min()), int(keys.max())
    k_rank = (n - 1) >> 1
    path, cls, refinements, pop, lane3, edge = 0, "equal", 0, n, False, None
    if kmn == kmx:
        med = kmn
    else:
        path = 1
        k = k_rank
        rebuild = conv
        if not conv:
            b, k, pop = _locate(np.bincount(np.minimum(np.maximum(first - lo0, 0) >> sh, nb - 1), minlength=nb), k)
            rebuild = speculative and b in (0, nb - 1)
            if rebuild:
                edge = "low" if b == 0 else "high"
        if rebuild:
            path = 18 if conv else 2
            lo0 = kmn
            sh = _shift(kmx - kmn, hb)
            b, k, pop = _locate(np.bincount((keys - lo0) >> sh, minlength=nb), k_rank)
        base = lo0 + (b << sh)
        cls = "direct"
        while sh > 0:
            r = keys - base
            member = (r >= 0) & ((r >> sh) == 0)
            if pop <= CAND_MAX:
                cls = "one_wave" if pop <= CAND_ONE else "all_waves"
                where = np.flatnonzero(member)
                lane3 = bool((np.bincount((where % tile) // 4) >= 3).any())
                base += int(np.sort(r[where])[k])
                break
            path |= 4
            refinements += 1
            sh2 = max(sh - hb, 0)
            b, k, pop = _locate(np.bincount(r[member] >> sh2, minlength=nb), k)
            base += b << sh2
            sh = sh2
            cls = "refined_to_one_key"
        med = base
    second, second_is_max = None, False
    if n % 2 == 0:
        if int((keys <= med).sum()) >= k_rank + 2:
            second = "equal"
        else:
            nxt = int(keys[keys > med].min())
            wave = (np.arange(n) % tile) // 256
            second = "same_wave" if np.intersect1d(wave[keys == nxt], wave[keys == med]).size else "other_wave"
            second_is_max = nxt == kmx
    return Plan(path, cls, refinements, pop, lane3, edge, second, second_is_max, med, conv)


def cells_of(plan):
    """A cell is (path word, class, 3+-member lane, edge).  A plan also stands for its cell with the lane left open (None) and
    for the one with class and lane left open, so that a requirement that names only part of a cell is a plain set member."""
    ranked = plan.cls in ("one_wave", "all_waves")
    return {(plan.path, plan.cls, plan.lane3 if ranked else None, plan.edge), (plan.path, plan.cls, None, plan.edge),
            (plan.path, None, None, plan.edge)}


def _required(threads, vpt):
    req = {
        (0, "empty", None, None), (0, "equal", None, None),
        (1, "one_wave", False, None), (1, "one_wave", True, None), (1, "all_waves", None, None),
        (5, "refined_to_one_key", None, None), (5, "all_waves", None, None),
        (18, None, None, None), (22, "refined_to_one_key", None, None),
    }
    # one negative sample at the end of a lognormal row: the exact range then spans both signs, 2^32 / 4096 keys per bin, and
    # from vpt = 4 on the median's bin holds more than CAND_MAX of the row's samples: one refinement, then ranking
    if vpt >= 4:
        req.add((22, "one_wave", None, None))
    if vpt >= 2:
        req.add((2, None, None, "low"))
    if vpt == 2:
        # the first tile is at least half the row: the lower median is never above the first tile's maximum, so it never sits
        # in the HIGH edge bin; a constant first tile puts it into bin 0 instead (low edge), which the exact range then has
        # to refine
        req.add((6, None, None, "low"))
    if vpt >= 3:
        req |= {(2, None, None, "high"), (2, "all_waves", None, "high"), (6, None, None, "high")}
    return frozenset(req)


REQUIRED = {shape: _required(*shape) for shape in REACHABLE}
# <256,1> never speculates (one tile holds the row): nothing can be clamped, so no rebuild but the re-keying one
IMPOSSIBLE = {(256, 1): frozenset({2, 6})}


def required(shape, parity):
    """REQUIRED for rows of one parity of n: an empty row has n = 0, which is even."""
    return REQUIRED[shape] - ({(0, "empty", None, None)} if parity else set())


# ---- recipes --------------------------------------------------------------------------------------------------------
PAD = np.float32(3.0e38)   # what a matrix holds past a row's count: a kernel that read it would get MAX and MED wrong


def _lognormal(rng, n):
    return rng.lognormal(1.0, 0.8, n).astype(np.float32)


def _decades(rng, n):
    return (10.0 ** rng.uniform(-30.0, 30.0, n)).astype(np.float32)


def lower_median(x):
    return np.sort(x)[(x.size - 1) >> 1]


def _copies(rng, x, c, start=0):
    """``c`` elements, drawn at random from ``start`` on, replaced by the row's lower median -- which stays the lower
    median."""
    start = min(start, x.size - 1)
    x[start + rng.choice(x.size - start, min(c, x.size - start), replace=False)] = lower_median(x)
    return x


def _copies_run(rng, x, c):
    """... at consecutive elements: three threads hold four members each."""
    at = 4 * int(rng.integers(0, max(x.size // 4 - 3, 1)))
    x[at:at + c] = lower_median(x)
    return x


def _copies_apart(rng, x, c, threads):
    """... one per thread."""
    v = lower_median(x)
    t = rng.choice(min(threads, max(x.size // 4, 1)), min(c, max(x.size // 4, 1)), replace=False)
    x[4 * t] = v
    return x


def _sparse_middle(x):
    """Samples within 2 % of the median moved 5 % further out (the median's rank stays): a bin is under 1 % wide, so the
    median's bin holds what a recipe puts there and nothing else.  The long rows of <1024,12> and <1024,16> fill a bin of a
    lognormal row with more than CAND_ONE samples; thinned out, they too are finished by one wave."""
    v = lower_median(x)
    x[(x > v) & (x < v * 1.02)] *= np.float32(1.05)
    x[(x < v) & (x > v / 1.02)] /= np.float32(1.05)
    return x


def _steps(rng, x, threads):
    """1000 distinct values a fixed number of f32 steps apart around the median of a 60-decade row.  The first histogram
    spans 2^31 keys, 2^32 where the estimate doubles tile 0's range: bins of 2^sh keys with sh = 31 or 32 less the
    histogram's bits.  They all fall into one bin (or two), one refinement leaves bins of 2^(sh - bits) keys, and the steps
    are chosen to put 128 values into such a bin: 2 keys for the 512- and 1024-thread shapes, 8 for <256,2>, 4 for <256,1>.
    Closer together they would fill a bin past CAND_MAX and the selection would go on to a single key."""
    hb = hist_bits(threads)
    d = 1 << ((32 if x.size > 4 * threads else 31) - 2 * hb - 7)
    c = min(1000, x.size)
    key = int(np.float32(lower_median(x)).view(np.uint32))
    vals = (key + d * (np.arange(c, dtype=np.int64) - c // 2)).astype(np.uint32).view(np.float32)
    x[rng.choice(x.size, c, replace=False)] = vals
    return x


def _first_tile(rng, n, threads, first):
    x = rng.uniform(100.0, 200.0, n).astype(np.float32)
    t = min(4 * threads, n)
    x[:t] = first if np.isscalar(first) else rng.uniform(first[0], first[1], t)
    return x


def _low_edge_by_clamp(rng, n, threads):
    """The estimate's origin clamped at key 0.  Tile 0 holds 0.0 and 1e6, so the estimate is [0, 2 * key(1e6)] and the exact
    range [0, key(1e6)]: bins half as wide.  The lower half of the row are denormals below the first exact bin's end, the
    median and nine neighbours denormals in the SECOND exact bin -- the first bin of the estimate.  It is the one way to a
    rebuild without refinement where tile 0 is more than half the row (<*,2> at odd n): there the median lies inside
    tile 0's range, and only the clamp at 0 lets that range start in bin 0."""
    s = 32 - hist_bits(threads)          # log2 of the estimate's bin width: 2 * key(1e6) needs all 32 bits
    if n < 32:
        return _lognormal(rng, n)
    low = rng.integers(1, 1 << (s - 1), (n - 1) // 2 - 4)
    mid = rng.integers(1 << (s - 1), 1 << s, 10)
    x = np.concatenate([low.astype(np.uint32).view(np.float32), mid.astype(np.uint32).view(np.float32),
                        rng.uniform(100.0, 200.0, n - low.size - 10).astype(np.float32)])
    rng.shuffle(x)
    x[0], x[1] = 0.0, 1e6
    return x


def _second_equal(rng, x):
    """rank k+1 holds the same value as rank k."""
    o = np.argsort(x, kind="stable")
    k = (x.size - 1) >> 1
    if k + 1 < x.size:
        x[o[k + 1]] = x[o[k]]
    return x


def _second_other_wave(rng, x):
    """rank k in wave 0 (element 0), rank k+1 in wave 1 (element 256)."""
    o = np.argsort(x, kind="stable")
    k = (x.size - 1) >> 1
    if x.size > 257:
        i, j = int(o[k]), int(o[k + 1])
        x[i], x[0] = x[0], x[i]
        j = i if j == 0 else j        # what element 0 held went to element i
        x[j], x[256] = x[256], x[j]
    return x


def _second_is_max(rng, x):
    """Everything above the median IS the maximum."""
    x[x > lower_median(x)] = x.max()
    return x


def _second_is_max_count(threads, stride):
    """That row has its own, short, even count, just past tile 0.  The reference for kernel rows sums the sorted row and its
    squared deviations sequentially in f32 (CuptiProfiler.cpp:63-69); n/2 EQUAL addends are each rounded the same way, up
    to half an ulp of the running sum, which biases the reference by up to n * 2^-25 of the result: 2.7e-4 of AVG and
    2.6e-4 of STD were seen at n = 40964 and 32769, past the 2e-4 that reference is compared within, while the kernel's
    mean was the f64 mean rounded to f32.  At n = 4098 the bias is at most 1.3e-4."""
    return min(stride, 4 * threads + 2)


def _signed_zeros(rng, n):
    return rng.choice(np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, 1e-38], dtype=np.float32), n)


class Recipe(NamedTuple):
    name: str
    make: object                  # (rng, n, threads) -> n samples
    moderate: bool = True         # finite samples over a moderate range: AVG and STD are compared as well
    count: object = None          # (threads, stride) -> the row's own count, whatever the launch's


def _neg_last(rng, n, t):
    x = _lognormal(rng, n)
    x[-1] = -x[-1]
    return x


RECIPES = (
    Recipe("n=0", lambda rng, n, t: _lognormal(rng, n), count=lambda t, s: 0),
    Recipe("n=1", lambda rng, n, t: _lognormal(rng, n), count=lambda t, s: 1),
    Recipe("n=2", lambda rng, n, t: _lognormal(rng, n), count=lambda t, s: min(2, s)),
    Recipe("n=tile", lambda rng, n, t: _lognormal(rng, n), count=lambda t, s: min(4 * t, s)),
    Recipe("n=tile+1", lambda rng, n, t: _lognormal(rng, n), count=lambda t, s: min(4 * t + 1, s)),
    Recipe("all 42", lambda rng, n, t: np.full(n, 42.0, np.float32)),
    Recipe("lognormal", lambda rng, n, t: _lognormal(rng, n)),
    Recipe("lognormal ascending", lambda rng, n, t: np.sort(_lognormal(rng, n))),
    Recipe("lognormal descending", lambda rng, n, t: np.sort(_lognormal(rng, n))[::-1].copy()),
    Recipe("12 medians in a run", lambda rng, n, t: _copies_run(rng, _lognormal(rng, n), 12)),
    Recipe("12 medians apart", lambda rng, n, t: _copies_apart(rng, _lognormal(rng, n), 12, t)),
    Recipe("12 medians in a run, sparse middle", lambda rng, n, t: _copies_run(rng, _sparse_middle(_lognormal(rng, n)), 12)),
    Recipe("12 medians apart, sparse middle", lambda rng, n, t: _copies_apart(rng, _sparse_middle(_lognormal(rng, n)), 12, t)),
    Recipe("100 medians", lambda rng, n, t: _copies(rng, _lognormal(rng, n), 100)),
    Recipe("300 medians", lambda rng, n, t: _copies(rng, _lognormal(rng, n), 300)),
    Recipe("300 medians, 60 decades", lambda rng, n, t: _copies(rng, _decades(rng, n), 300), moderate=False),
    Recipe("1000 steps, 60 decades", lambda rng, n, t: _steps(rng, _decades(rng, n), t), moderate=False),
    Recipe("one negative at the end", _neg_last),
    Recipe("lognormal, negated", lambda rng, n, t: -_lognormal(rng, n)),
    Recipe("300 medians, negated", lambda rng, n, t: -_copies(rng, _lognormal(rng, n), 300)),
    Recipe("tile 0 = 1e6", lambda rng, n, t: _first_tile(rng, n, t, 1e6)),
    Recipe("tile 0 ~ 1e6", lambda rng, n, t: _first_tile(rng, n, t, (1e6, 1.001e6))),
    Recipe("tile 0 = 1", lambda rng, n, t: _first_tile(rng, n, t, 1.0)),
    Recipe("tile 0 ~ 1", lambda rng, n, t: _first_tile(rng, n, t, (1.0, 1.001))),
    Recipe("tile 0 ~ 1, 300 medians", lambda rng, n, t: _copies(rng, _first_tile(rng, n, t, (1.0, 1.001)), 300, 4 * t)),
    Recipe("tile 0 ~ 1, 100 medians", lambda rng, n, t: _copies(rng, _first_tile(rng, n, t, (1.0, 1.001)), 100, 4 * t)),
    Recipe("tile 0 from 0 to 1e6, median a denormal", _low_edge_by_clamp, moderate=False),
    Recipe("second middle equal", lambda rng, n, t: _second_equal(rng, _lognormal(rng, n))),
    Recipe("second middle in another wave", lambda rng, n, t: _second_other_wave(rng, _lognormal(rng, n))),
    Recipe("second middle is the maximum", lambda rng, n, t: _second_is_max(rng, _lognormal(rng, n)),
           count=_second_is_max_count),
    Recipe("signed zeros and denormals", lambda rng, n, t: _signed_zeros(rng, n), moderate=False),
)

COUNTS = (0, 1, 3)   # a launch's count is the stride less one of these


def matrix(stride, less):
    """All recipes as one [rows, stride] matrix for the launch shape of ``stride``, with each row's count (stride - less, or
    the recipe's own) and its plan."""
    threads, vpt = pick(stride)
    m = np.full((len(RECIPES), stride), PAD, dtype=np.float32)
    counts = np.empty(len(RECIPES), dtype=np.uint32)
    plans = []
    for i, rec in enumerate(RECIPES):
        n = rec.count(threads, stride) if rec.count else stride - less
        rng = np.random.default_rng([stride, less, i])
        m[i, :n] = rec.make(rng, n, threads) if n else []
        counts[i] = n
        plans.append(selection_plan(m[i], n, threads, vpt))
    return m, counts, plans
