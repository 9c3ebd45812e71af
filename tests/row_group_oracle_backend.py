"""Row-family scores per peer group for the CPU checker backend, the NumPy restatement the tests compare against, and the
small exact window they play -- TEST INFRASTRUCTURE, lives outside the product.

``row_group_records`` restates the contract of include/nvrx_straggler.h (``nvrx_rowfam_group_score``) in NumPy and plain
Python: block A is ``peer_oracle_backend.peer_columns`` over plane 0, block B one f64 quotient per slot and, for the GPU slot,
a sequential f64 sum in ascending kernel id.  It shares nothing with the kernels.  ``RowGroupOracleBackend`` is
``PeerHistoryOracleBackend`` plus the four ``*_group_score`` methods built on it (it lacks the slack scores per peer group); ``CountingRowGroupBackend`` has
grouped methods that only count and raise.

The window (``make`` / ``report``) is tests/row_family_script.py's, doubled: four logical ranks folded into one process, stages
``(0, 0, 1, 1)`` at 1000 and 1500, 64-deep rings, integer samples.  Rank 1 carries the three planted patterns alone (step,
beat, stretch); BOTH ranks of stage 1 share a beat (a stage-local stall), and rank 3 alone has the stretch.  Each stage also
runs a kernel of its own (``gemm_a`` / ``gemm_b``, flat): what ``peer_groups="auto"`` tells the stages apart by, and columns
that half of the ranks lack.

``RowGroupOracleBackend`` has no ``slack_group_score``: the checker that serves a report with every option on is
tests/full_oracle_backend.py's ``FullOracleBackend``, and the all-options run is tests/full_report_script.py.
"""
import numpy as np

from peer_history_oracle_backend import PeerHistoryOracleBackend
from peer_oracle_backend import peer_columns

NAN32 = np.float32(np.nan)
FAMILY_NAMES = ("tail", "onset", "period", "episode")
PLANES = {"tail": 1, "onset": 6, "period": 7, "episode": 7}


def row_group_records(planes0, table, K, S, arrays, G, first_rank=0, n_ranks=None, min_ranks=2):
    """``(cols [G, K+S, 4] uint32, scores [n_ranks, 1 + S] f32)`` of plane 0 ``planes0`` [R, K+S] f32, the weights of
    ``table`` [R, L] (None at K = 0) and the array ``group[R] | members[R] | start[G+1]``."""
    V = np.ascontiguousarray(planes0, dtype=np.float32)
    R, KS = V.shape[0], K + S
    n_ranks = R - first_rank if n_ranks is None else n_ranks
    cols = peer_columns(V, K, S, arrays, G, min_ranks)
    floor = cols[:, :, 0].view(np.float32)
    present = cols[:, :, 1]
    out = np.full((n_ranks, 1 + S), NAN32, dtype=np.float32)
    for i in range(n_ranks):
        r = first_rank + i
        g = int(arrays[r])
        if not 0 <= g < G:
            continue
        sw = sq = np.float64(0.0)
        n = 0
        for c in range(KS):
            v = V[r, c]
            if not v >= 0 or int(present[g, c]) < min_ranks:
                continue
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                q = np.float64(floor[g, c]) / np.float64(v)
                if c >= K:
                    out[i, 1 + c - K] = np.float32(q)
                else:
                    w = np.float64(table[r, 2 * KS + c])
                    sq = sq + w * q
                    sw = sw + w
                    n += 1
        if n:
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                out[i, 0] = np.float32(sq / sw)
    return cols, out


class _OracleRowGroup:
    def __init__(self, rec, G, first_rank, n_ranks, min_ranks):
        self._rec = rec
        self.G, self.first_rank, self.n_ranks, self.min_ranks = G, first_rank, n_ranks, min_ranks
        self.reads = 0

    def records(self):
        self.reads += 1
        return self._rec


class RowGroupOracleBackend(PeerHistoryOracleBackend):
    """The CPU checker up to the peer-score history plus the row families per peer group (computed at enqueue time).  It
    lacks ``slack_group_score``: a report with ``slack_peer_groups`` too needs ``full_oracle_backend.FullOracleBackend``."""

    name = "oracle-test+row-group"

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.row_group_calls = []    # family names, in call order
        self.row_group_args = []
        self.row_group_handles = {}  # family name -> handles

    def _group_score(self, fam, ws, planes, table, groups, first_rank, n_ranks, min_ranks):
        n_ranks = ws.R - first_rank if n_ranks is None else n_ranks
        assert groups.R == ws.R, (groups.R, ws.R)
        KS, P = ws.K + ws.S, PLANES[fam]
        self.row_group_calls.append(fam)
        self.row_group_args.append((fam, ws.R, ws.K, ws.S, groups.G, first_rank, n_ranks, min_ranks))
        O = planes.numpy().copy().reshape(ws.R, P, KS)
        cols, sc = row_group_records(O[:, 0, :], table.numpy().copy(), ws.K, ws.S, groups.host, groups.G, first_rank, n_ranks,
                                     min_ranks)
        part = O[first_rank : first_rank + n_ranks]
        h = _OracleRowGroup((part.reshape(n_ranks, KS) if P == 1 else part, sc, cols), groups.G, first_rank, n_ranks, min_ranks)
        self.row_group_handles.setdefault(fam, []).append(h)
        return h

    def tail_group_score(self, ws, tails, table, groups, first_rank=0, n_ranks=None, min_ranks=2, q_ppm=0):
        return self._group_score("tail", ws, tails, table, groups, first_rank, n_ranks, min_ranks)

    def onset_group_score(self, ws, onsets, table, groups, first_rank=0, n_ranks=None, min_ranks=2):
        return self._group_score("onset", ws, onsets, table, groups, first_rank, n_ranks, min_ranks)

    def period_group_score(self, ws, periods, table, groups, first_rank=0, n_ranks=None, min_ranks=2):
        return self._group_score("period", ws, periods, table, groups, first_rank, n_ranks, min_ranks)

    def episode_group_score(self, ws, episodes, table, groups, first_rank=0, n_ranks=None, min_ranks=2):
        return self._group_score("episode", ws, episodes, table, groups, first_rank, n_ranks, min_ranks)


class CountingRowGroupBackend(PeerHistoryOracleBackend):
    """The checker with everything else working -- the job-wide row families and the peer scores included -- and grouped
    row-family methods that only count and raise."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.row_group_calls = 0

    def _grouped(self, *a, **kw):
        self.row_group_calls += 1
        raise AssertionError("a *_group_score() method was called although row_peer_groups is off")

    tail_group_score = onset_group_score = period_group_score = episode_group_score = _grouped


# ---- the small exact window -------------------------------------------------------------------------------------------------
LOCAL_RANKS, RING_CAP, ROWS = 4, 64, ("step", "beat", "stretch")
STAGE_KERNELS = ("gemm_a", "gemm_b")  # always kernel rows; stage s runs STAGE_KERNELS[s] only
LABELS = (0, 0, 1, 1)
STAGE_US = (1000.0, 1000.0, 1500.0, 1500.0)
OPTIONS = dict(tail_quantile=0.7, onset_detection=True, period_detection=True, episode_detection=True)


def pushes(window: int = 0):
    """``{(row name, logical rank): samples to push}`` of one window (``window`` scales it: windows differ, patterns do not)."""
    out = {}
    for r, us in enumerate(STAGE_US):
        base = np.float32(us * (1 + window))
        flat = np.full(RING_CAP, base, dtype=np.float32)
        step, beat, stretch = flat, flat, flat
        if r == 1:
            step = np.full(80, base, dtype=np.float32)  # (80 into a ring of 64: it wraps)
            step[-16:] *= np.float32(2.0)
        if r in (1, 2, 3):
            beat = flat.copy()
            beat[3::4] *= np.float32(1.5)
        if r in (1, 3):
            stretch = flat.copy()
            stretch[30:42] *= np.float32(1.6)
        out.update({("step", r): step, ("beat", r): beat, ("stretch", r): stretch})
        out[(STAGE_KERNELS[LABELS[r]], r)] = np.full(RING_CAP, np.float32(100.0 * (1 + LABELS[r]) * (1 + window)), dtype=np.float32)
    return out


def make(be, kernels=(), peer_groups=LABELS, local_ranks=LOCAL_RANKS, spare_rows=0, **options):
    """``(generator, rings, rows)`` on the active backend ``be``: the rows named in ``kernels`` are kernel rows, the others
    section rows; ``options`` that switch no family on come on top of all four families with ``row_peer_groups``;
    ``local_ranks`` of the four logical ranks live in this process."""
    from nvrx_straggler.reporting import ReportGenerator

    if not any(name in options for name in OPTIONS):
        options = dict(OPTIONS, row_peer_groups=True, **options)
    options.setdefault("gather_on_rank0", True)
    gen = ReportGenerator(["relative_perf_scores"], node_name="n", peer_groups=peer_groups, **options)
    rings = be.make_rings(local_ranks, len(ROWS) + len(STAGE_KERNELS) + spare_rows, RING_CAP)
    rows = {name: rings.row_for(int(name in kernels or name in STAGE_KERNELS), name) for name in ROWS + STAGE_KERNELS}
    return gen, rings, rows


def report(gen, rings, rows, kernels=(), window: int = 0, local_ranks=LOCAL_RANKS, first_rank: int = 0):
    """Fill one window -- this process holding the logical ranks ``[first_rank, first_rank + local_ranks)`` --, report it,
    empty the rings.  The report is returned unread."""
    for (name, r), values in pushes(window).items():
        if first_rank <= r < first_rank + local_ranks:
            rings.push_many(rows[name], values, lr=r - first_rank)
    kernels = tuple(kernels) + STAGE_KERNELS
    rep = gen.generate_report_from_rings(rings, {n: r for n, r in rows.items() if n not in kernels},
                                         {n: r for n, r in rows.items() if n in kernels}, local_ranks=local_ranks)
    rings.reset()
    return rep


def family_scores(rep):
    return {fam: getattr(rep, fam + "_scores")() for fam in FAMILY_NAMES}


def same(a, b) -> bool:
    """``a == b`` for a report's nested dicts and lists, with NaN equal to NaN."""
    if isinstance(a, dict) and isinstance(b, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and isinstance(b, float) and a != a and b != b:
        return True
    return type(a) is type(b) and a == b


NEW_KEYS = ("peer_groups", "min_peers", "groups", "group_of", "unrated_ranks", "section_reference", "kernel_reference")
