"""One small window that every row family has something to say about, for tests/test_row_families_host.py (CPU oracle) and
tests/test_gpu_row_families.py (HIP engine): two logical ranks folded into one process, 64-deep rings, three section rows.

Rank 0 is flat.  Rank 1 carries one planted pattern per row, each meant for ONE family:

* ``step``    the last 16 of the window's 64 samples are 2 x slower: an onset (the 8-sample minimum segment binds: 5 % of 64
              is 3.2 samples).  80 samples are pushed into this row, so the ring has wrapped (``start != 0``) and the window
              is the last 64;
* ``beat``    every 4th sample is 1.5 x slower: a period of 4 (the largest candidate is n / 4 = 16, not ``period_max``);
* ``stretch`` samples 30 .. 41 are 1.6 x slower: an episode of 12 samples (the 8-sample minimum length binds: 0.5 % of 64 is
              0.32 samples).

The tail quantile is 0.7: every pattern touches at most a quarter of its row, so no rank's 0.7-quantile moves and the tail
family -- which has no row of its own -- flags nobody.  Samples are integers far below 2^24: every sum is exact in f32 and f64.
"""
import numpy as np

LOCAL_RANKS, RING_CAP, ROWS = 2, 64, ("step", "beat", "stretch")
MEANT_FOR = {"onset": "step", "period": "beat", "episode": "stretch"}  # family -> the row whose pattern it is to find
OPTIONS = dict(tail_quantile=0.7, onset_detection=True, period_detection=True, episode_detection=True)
FLAT = 1000.0


def pushes(window: int = 0):
    """``{(row name, logical rank): samples to push}`` of one window (``window`` scales it: windows differ, patterns do not)."""
    base = np.float32(FLAT * (1 + window))
    flat = np.full(RING_CAP, base, dtype=np.float32)
    step = np.full(80, base, dtype=np.float32)
    step[-16:] *= np.float32(2.0)
    beat = flat.copy()
    beat[3::4] *= np.float32(1.5)
    stretch = flat.copy()
    stretch[30:42] *= np.float32(1.6)
    out = {(name, 0): flat for name in ROWS}
    out.update({("step", 1): step, ("beat", 1): beat, ("stretch", 1): stretch})
    return out


def fill(rings, rows, window: int = 0) -> None:
    for (name, lr), values in pushes(window).items():
        rings.push_many(rows[name], values, lr=lr)


def make(be, kernels=(), **options):
    """``(generator, rings, rows)`` on the active backend ``be``: the rows named in ``kernels`` are kernel rows, the others
    section rows; ``options`` instead of all four families."""
    from nvrx_straggler.reporting import ReportGenerator

    gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=True, node_name="n", **(options or OPTIONS))
    rings = be.make_rings(LOCAL_RANKS, len(ROWS), RING_CAP)
    rows = {name: rings.row_for(int(name in kernels), name) for name in ROWS}
    return gen, rings, rows


def report(gen, rings, rows, kernels=(), window: int = 0):
    """Fill one window, report it, empty the rings.  The report is returned unread."""
    fill(rings, rows, window)
    rep = gen.generate_report_from_rings(rings, {n: r for n, r in rows.items() if n not in kernels},
                                         {n: r for n, r in rows.items() if n in kernels}, local_ranks=LOCAL_RANKS)
    rings.reset()
    return rep


def same(a, b) -> bool:
    """``a == b`` for a report's nested dicts, with NaN equal to NaN."""
    if isinstance(a, dict) and isinstance(b, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, float) and isinstance(b, float) and a != a and b != b:
        return True
    return type(a) is type(b) and a == b
