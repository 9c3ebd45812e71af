"""The shapes, node layouts and tables of the node-score parity tests -- TEST INFRASTRUCTURE.  tests/test_gpu_node.py runs the
kernels on them; tests/test_node_host.py checks, with the NumPy restatement alone, that every case holds what the GPU test
relies on (``case_properties``).

A case is (R, K, S, layout).  The shapes sit at the geometry's edges: the 64-column tile, R = 64 | 65 (one fused launch | two
launches), a node above a wave, more than 64 nodes in the across-node select, a part of 4097 columns (the rank kernel's
re-reading form).  ``mod:N`` and ``65+35`` put a node's members apart: a kernel that reads row ``s + i`` instead of
``members[s + i]`` passes every ``block:N`` case."""
import numpy as np

from pace_group_oracle_backend import threshold
from score_cases import random_table

CASES = [(1, 3, 0, "one"), (2, 2, 2, "singletons"), (8, 1, 1, "block:4"), (8, 63, 3, "block:2"), (8, 64, 0, "mod:2"),
         (8, 65, 2, "mod:2"), (12, 5, 3, "1+3+8"), (64, 17, 33, "block:8"), (65, 70, 5, "block:5"), (100, 7, 9, "65+35"),
         (130, 3, 2, "singletons"), (1025, 3, 2, "mod:17"), (4, 4097, 0, "block:2")]
THRESHOLDS = ((2, 3), (1, 1))  # (min_members, min_nodes)
COLUMN_KINDS = ("absent_in_node", "only_in_node", "nan_inf_zero", "equal", "ties", "at_members", "below_members", "at_nodes",
                "below_nodes")
NAN_BITS = 0x7FC00000


def labels_of(R, layout):
    kind, _, num = layout.partition(":")
    if kind == "one":
        return [0] * R
    if kind == "singletons":
        return list(range(R))
    if kind == "block":
        return [r // int(num) for r in range(R)]
    if kind == "mod":
        return [r % int(num) for r in range(R)]
    if layout == "1+3+8":
        assert R == 12
        return [0] + [1] * 3 + [2] * 8
    assert layout == "65+35" and R == 100
    labels = np.zeros(R, dtype=int)
    labels[np.linspace(1, 98, 35).astype(int)] = 1  # 35 ranks spread among the other 65
    assert labels.sum() == 35
    return labels.tolist()


def _special_column(T, rng, c, kind, K, S, labels, j):
    """One column made special: within node ``j`` (the other nodes keep ordinary values), or across the nodes."""
    R, KS = T.shape[0], K + S
    G = int(labels.max()) + 1
    members = np.flatnonzero(labels == j % G)
    n = len(members)
    col = rng.lognormal(1.0, 0.5, R).astype(np.float32)
    col[rng.random(R) < 0.15] = -1.0
    need = threshold(2, 1, n)
    if kind == "absent_in_node":
        col[members] = -1.0
    elif kind == "only_in_node":
        mine = col[members]
        col[:] = -1.0
        col[members] = np.abs(mine)
    elif kind == "nan_inf_zero":  # quotients of +inf and 0, and a NaN that is absent
        col[members] = rng.lognormal(1.0, 0.5, n).astype(np.float32)
        col[members[0]] = 0.0
        col[members[-1]] = np.inf if n > 1 else 0.0
        if n > 2:
            col[members[n // 2]] = np.nan
    elif kind == "equal":  # the same value on every rank: every node's median and the centre are it
        col[:] = np.float32(3.25)
    elif kind == "ties":  # most ranks hold the median's value: nodes tie with the centre
        col[:] = rng.choice(np.array([1.5, 2.0, 2.0, 2.0, 2.5], dtype=np.float32), R)
    elif kind in ("at_members", "below_members"):  # exactly as many present members as a pair needs at 2, and one fewer
        keep = min(n, need if kind == "at_members" else need - 1)
        col[members] = -1.0
        col[rng.permutation(members)[:keep]] = rng.lognormal(1.0, 0.5, keep).astype(np.float32)
    elif kind in ("at_nodes", "below_nodes"):  # exactly as many nodes with all their members as a column needs at 3, one fewer
        keep = min(G, 3) - (kind == "below_nodes")
        with_data = (j + np.arange(keep)) % G
        col[:] = np.where(np.isin(labels, with_data), rng.lognormal(1.0, 0.5, R), -1.0).astype(np.float32)
    T[:, c] = col
    if c < K:
        with np.errstate(invalid="ignore"):
            T[:, 2 * KS + c] = np.where(col >= 0, rng.uniform(1, 1000, R), 0.0).astype(np.float32)


def tables(R, K, S, labels):
    """The tables of one case: ``random_table`` with 15 % of the medians absent, every NODE scaled to a pace of its own and
    every rank a little around it, plus the special columns, each within one node in turn, spread over the columns (a case with
    fewer columns than kinds gets several tables)."""
    rng = np.random.default_rng(R * 1000 + K + S)
    KS = K + S
    labels = np.asarray(labels)
    G = int(labels.max()) + 1
    todo = list(enumerate(COLUMN_KINDS))
    while todo:
        T = random_table(rng, R, K, S)
        scale = rng.permutation(np.linspace(0.7, 1.4, G).astype(np.float32))[labels] * rng.uniform(0.97, 1.03, R).astype(np.float32)
        T[:, :KS] = np.where(T[:, :KS] >= 0, T[:, :KS] * scale[:, None], T[:, :KS])
        take, todo = todo[:KS], todo[KS:]
        cols = np.linspace(0, KS - 1, len(take)).astype(int) if len(take) > 1 else [KS // 2]
        for c, (j, kind) in zip(cols, take):
            _special_column(T, rng, int(c), kind, K, S, labels, j)
        yield T


def case_properties(results, G):
    """What a case must hold, from the restatement's ``(pairs, cols, nodes, ranks, ...)`` of all its tables and thresholds:
    ``rated`` -- some node has an eligible column; ``pair_unreferenced`` -- a pair with data and no reference;
    ``column_short`` -- a column with referenced nodes but fewer than ``min_nodes``."""
    rated = pair_unreferenced = column_short = False
    for pairs, cols, nodes, *_ in results:
        rated = rated or bool((nodes[:, :, 2] > 0).any())
        pair_unreferenced = pair_unreferenced or bool(((pairs[:, :, 0] == NAN_BITS) & (pairs[:, :, 1] > 0)).any())
        column_short = column_short or bool(((cols[:, 0] == NAN_BITS) & (cols[:, 1] > 0)).any())
    return {"rated": rated, "pair_unreferenced": pair_unreferenced, "column_short": column_short}


def check_properties(props, labels):
    """Every case rates some node.  A pair with data and no reference needs a node of at least two members (one of one member
    is referenced by its only value: the clamp of ``min_members`` to the node's size), so the cases of single-member nodes
    must NOT hold one.  A column with referenced nodes but fewer than ``min_nodes`` is asked of three nodes or more."""
    sizes = np.bincount(np.asarray(labels))
    assert props["rated"], props
    assert props["pair_unreferenced"] == bool(sizes.max() >= 2), (props, sizes.max())
    if len(sizes) >= 3:
        assert props["column_short"], props
