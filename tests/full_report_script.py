"""The all-options run: ONE pipeline job with every follow-up result a report can carry switched on, shared by the CPU tests
(tests/test_full_report_host.py, on ``full_oracle_backend.FullOracleBackend``) and the GPU tests
(tests/test_gpu_full_report.py, on the HIP engine) -- TEST INFRASTRUCTURE, lives outside the product.  A feature that lands
later gets an entry in ``FEATURES`` (and its options in that entry), not another sibling checker and another script.

The job: ``ranks`` logical ranks (8; 66 for the size past a wave) folded into processes, two pipeline stages of ``ranks / 2``
(the labels ``peer_groups`` gets), nodes of two ranks (``node_groups="block:2"``), rings 256 deep.  Section rows ``step``,
``beat`` and ``stretch``; kernel rows one GEMM per stage, one kernel every rank runs (without it no kernel is common to all
ranks and the job-wide GPU score, with its attribution and its history, is NaN everywhere) and the two collective kernels of
tests/slack_group_oracle_backend.py, of which only the compute kernels are handed over as kernel rows (the slack step finds
the collective rows in the rings' own table, as ``play_stages`` does).  Six windows that differ by scale, by one step and by
one drift, their patterns never:

=========  ==========================  ==========================================================================================
plant      rank (8 ranks / in general)  what it does
=========  ==========================  ==========================================================================================
onset      1                            ``step`` gets 320 samples into a ring of 256 (it wraps: the start-offset path), the last 64 x2
drift      2                            ``step`` x (1 + 0.08 w) in window w: a score that falls from report to report (trends)
tail       3                            51 scattered samples of ``step`` x1.8 (a fifth of the window)
pace       4 = half                     its GEMM and the common kernel are 6 % slower (pace, attribution, robust)
history    5 = half + 1                 ``step`` x1.6 from window 3 on (score history, peer history, robust)
late       6 = half + 2                 arrives 300 us late at every all-reduce of its stage (slack); ``beat`` x1.5 every 4th sample
stretch    7 = half + 3                 samples 100..149 of ``stretch`` x1.6 (episode)
=========  ==========================  ==========================================================================================

``variant=True`` is the job whose inferred groups change: a third GEMM name is a kernel row from the start (so the table's shape
never changes), and rank 2 runs it instead of its stage's GEMM in window 3 only -- with ``peer_groups="auto"`` the group count
goes 2 -> 3 -> 2.
"""
import numpy as np

from row_group_oracle_backend import same  # noqa: F401  (the tests' "exactly": NaN equal to NaN)
from slack_group_oracle_backend import ALLREDUCE, SENDRECV, STAGE_GEMMS, stage_scenario

RANKS, RING_CAP, ROWS_PER_RANK, WINDOWS, CALLS = 8, 256, 10, 6, 200
SECTIONS = ("step", "beat", "stretch")
ALT_GEMM = "gemm_stage0_alt<bf16>"  # (the variant's third GEMM)
COMMON = "adamw_step<f32>"  # (the kernel every rank runs: a job-wide GPU score covers the kernels all ranks have)
STAGE_US = (1000.0, 1200.0)
HISTORY_FROM, VARIANT_WINDOW, VARIANT_RANK = 3, 3, 2
FAMILY_NAMES = ("tail", "onset", "period", "episode")


def labels(ranks=RANKS):
    return tuple(r // (ranks // 2) for r in range(ranks))


def plants(ranks=RANKS):
    half = ranks // 2
    return {"onset": 1, "drift": 2, "tail": 3, "pace": half, "history": half + 1, "late": half + 2, "beat": half + 2,
            "stretch": half + 3}


_PUSHES = {}


def pushes(window=0, ranks=RANKS, variant=False):
    """``{(row name, logical rank): f32 samples to push}`` of one window (computed once per argument list, never changed)."""
    key = (window, ranks, variant)
    if key in _PUSHES:
        return _PUSHES[key]
    stage, who, scale = labels(ranks), plants(ranks), np.float32(1 + window)
    _, _, allreduce, bubble = stage_scenario(stage, late_rank=who["late"], calls=CALLS)
    tail_at = np.random.default_rng(5).permutation(RING_CAP)[:51]
    out = {}
    for r in range(ranks):
        base = np.float32(STAGE_US[stage[r]]) * scale
        flat = np.full(RING_CAP, base, dtype=np.float32)
        step, beat, stretch = flat.copy(), flat, flat
        if r == who["onset"]:
            step = np.full(RING_CAP + 64, base, dtype=np.float32)
            step[-64:] *= np.float32(2.0)
        if r == who["drift"]:
            step *= np.float32(1.0 + 0.08 * window)
        if r == who["tail"]:
            step[tail_at] *= np.float32(1.8)
        if r == who["history"] and window >= HISTORY_FROM:
            step *= np.float32(1.6)
        if r == who["beat"]:
            beat = flat.copy()
            beat[3::4] *= np.float32(1.5)
        if r == who["stretch"]:
            stretch = flat.copy()
            stretch[100:150] *= np.float32(1.6)
        gemm = np.full(CALLS, np.float32(100.0 * (1 + stage[r])) * scale, dtype=np.float32)
        common = np.full(CALLS, np.float32(50.0) * scale, dtype=np.float32)
        if r == who["pace"]:
            gemm *= np.float32(1.06)
            common *= np.float32(1.06)
        name = STAGE_GEMMS[stage[r]]
        if variant and r == VARIANT_RANK and window == VARIANT_WINDOW:
            name = ALT_GEMM
        out.update({("step", r): step, ("beat", r): beat, ("stretch", r): stretch, (name, r): gemm,
                    (COMMON, r): common, (ALLREDUCE, r): allreduce[r] * scale, (SENDRECV, r): bubble[r] * scale})
    _PUSHES[key] = out
    return out


# ---- the features: the smallest option set that switches each on (prerequisites included), its reader, its raw handles ---------
def _peer(ranks):
    return {"peer_groups": labels(ranks)}


def _family(option, value):
    return lambda ranks: dict(_peer(ranks), row_peer_groups=True, **{option: value})


FEATURES = {
    # name: (options(ranks), reader(report), the report's slots that hold the raw handles behind it)
    "scores": (lambda ranks: {}, lambda rep: {"gpu_relative": dict(rep.gpu_relative_perf_scores),
                                              "section_relative": {n: dict(v) for n, v in rep.section_relative_perf_scores.items()}}, ()),
    "attribution": (lambda ranks: {"kernel_attribution": 2}, lambda rep: rep.explain_gpu_scores(), ("_attr",)),
    "robust": (lambda ranks: {"robust_scores": True, "robust_floor": 0.01}, lambda rep: rep.robust_scores(), ("_robust",)),
    "tail": (_family("tail_quantile", 0.9), lambda rep: rep.tail_scores(), ("_tail",)),
    "onset": (_family("onset_detection", True), lambda rep: rep.onset_scores(), ("_onset",)),
    "period": (_family("period_detection", True), lambda rep: rep.period_scores(), ("_period",)),
    "episode": (_family("episode_detection", True), lambda rep: rep.episode_scores(), ("_episode",)),
    "peer": (_peer, lambda rep: rep.peer_scores(), ("_peer",)),
    "peer_history": (lambda ranks: dict(_peer(ranks), peer_history=8, peer_trends=True, trend_min_reports=4),
                     lambda rep: {"history": rep.peer_history(), "trends": rep.peer_trends()}, ("_peer_history", "_peer_trends")),
    "pace": (lambda ranks: dict(_peer(ranks), pace_scores=True, pace_peer_groups=True, pace_min_columns=1),
             lambda rep: rep.pace_scores(), ("_pace",)),
    "node": (lambda ranks: {"node_scores": True, "node_groups": "block:2", "node_min_columns": 1},
             lambda rep: rep.node_scores(), ("_node",)),
    "history": (lambda ranks: {"score_history": 8, "score_trends": True, "trend_min_reports": 4},
                lambda rep: {"history": rep.score_history(), "trends": rep.score_trends()}, ("_history", "_trends")),
    "slack": (lambda ranks: dict(_peer(ranks), collective_slack=True, slack_peer_groups=True),
              lambda rep: rep.slack_scores(), ("_slack",)),
    # by design work_groups() gains the labelled comparison ("label_conflicts") when peer_groups labels are set
    # (ReportGenerator._follow_ups): "alone" is work_groups=True WITH the labels
    "work": (lambda ranks: dict(_peer(ranks), work_groups=True), lambda rep: rep.work_groups(), ("_work",)),
}

# the identify_* calls the plants are meant for: feature -> (method name, ...)
IDENTIFY = {
    "robust": ("identify_robust_stragglers",), "tail": ("identify_tail_stragglers",), "onset": ("identify_onset_stragglers",),
    "period": ("identify_period_stragglers",), "episode": ("identify_episode_stragglers",),
    "peer": ("identify_peer_stragglers",), "pace": ("identify_pace_stragglers",),
    "peer_history": ("identify_persistent_peer_stragglers", "identify_declining_peer_stragglers"),
    "history": ("identify_persistent_stragglers", "identify_declining_stragglers"),
    "slack": ("identify_slack_stragglers",),
}


def options_of(features=None, ranks=RANKS, peer_groups=None):
    """The options of ``features`` (None: all of them) together; ``peer_groups`` replaces the labels where they are set."""
    out = {}
    for name in FEATURES if features is None else features:
        out.update(FEATURES[name][0](ranks))
    if peer_groups is not None and "peer_groups" in out:
        out["peer_groups"] = peer_groups
    return out


def read(rep, features=None):
    """``{feature: what its reader says}`` of one report."""
    return {name: FEATURES[name][1](rep) for name in (FEATURES if features is None else features)}


def named(found):
    """Ranks named anywhere in an ``identify_*`` result (sets of StragglerId, bare or per section)."""
    ranks = set()
    for v in found.values():
        for group in (v.values() if isinstance(v, dict) else [v]):
            ranks |= {s.rank for s in group}
    return sorted(ranks)


def identified(rep, features=None):
    """``{identify method: ranks it names}`` of one report."""
    return {m: named(getattr(rep, m)()) for name in (IDENTIFY if features is None else features) for m in IDENTIFY.get(name, ())}


def raw(rep, features=None):
    """``{feature: [arrays]}``: the records behind every feature of an UNREAD report, through the handles' own ``records()``
    (as tests/test_gpu_row_families.py::_handles does); features without a handle are left out."""
    out = {}
    for name in FEATURES if features is None else features:
        arrays = []
        for slot in FEATURES[name][2]:
            rec = rep.__dict__[slot].handle.records()
            arrays += [np.ascontiguousarray(a) for a in (rec if isinstance(rec, (tuple, list)) else (rec,))]
        if arrays:
            out[name] = arrays
    return out


class Job:
    """One generator with its rings and its (stable) tables of rows on the active backend ``be``: the logical ranks
    ``[first_rank, first_rank + local_ranks)`` of ``ranks`` live in this process."""

    def __init__(self, be, features=None, ranks=RANKS, local_ranks=None, first_rank=0, variant=False,
                 rows_per_rank=ROWS_PER_RANK, **options):
        from nvrx_straggler.reporting import ReportGenerator

        self.ranks, self.local_ranks, self.first_rank, self.variant = ranks, ranks if local_ranks is None else local_ranks, first_rank, variant
        opts = options_of(features, ranks, options.pop("peer_groups", None))
        opts.update(options)
        opts.setdefault("gather_on_rank0", True)
        self.gen = ReportGenerator(["relative_perf_scores"], node_name="n", **opts)
        self.rings = be.make_rings(self.local_ranks, rows_per_rank, RING_CAP)
        self.section_rows = {name: self.rings.row_for(0, name) for name in SECTIONS}
        gemms = STAGE_GEMMS + (COMMON,) + ((ALT_GEMM,) if variant else ())
        self.rows = dict(self.section_rows, **{k: self.rings.row_for(1, k) for k in gemms + (ALLREDUCE, SENDRECV)})
        self.kernel_rows = {k: self.rows[k] for k in gemms}  # (the compute kernels only)

    def report(self, window):
        """Fill one window, report it, empty the rings.  The report is returned unread."""
        lo, hi = self.first_rank, self.first_rank + self.local_ranks
        for (name, r), values in pushes(window, self.ranks, self.variant).items():
            if lo <= r < hi:
                self.rings.push_many(self.rows[name], values, lr=r - lo)
        rep = self.gen.generate_report_from_rings(self.rings, self.section_rows, self.kernel_rows, local_ranks=self.local_ranks)
        self.rings.reset()
        return rep

    def close(self):
        self.gen.close()
        self.rings.close()


# ---- what the readers' mappings are keyed by ----------------------------------------------------------------------------------
# Every mapping with integer keys in a reader's result is listed here by the key it sits under -- directly ({rank: ...}) or one
# level below ({row name: {rank: ...}}) -- with what its integers are.  ``by_rank`` and ``per_rank`` decide by this table alone
# and REFUSE a mapping that is not in it: a reader that gains a key cannot go uncompared quietly, it has to be classified.
KEYED = {
    "ranks": "rank", "relative": "rank", "gpu_relative": "rank", "gpu_scores": "rank", "gpu_ratio": "rank", "gpu_z": "rank",
    "group_of": "rank to group",                       # {rank: label}
    "node_of": "every rank",                           # {rank: node} of ALL ranks, also in a report that covers a part of them
    "groups": "group", "per_group": "group",           # {label: ...}
    "nodes": "other", "node_scores": "other", "per_node": "other", "columns": "other", "label_conflicts": "other",
}
KEYED_BELOW = {
    **{f"{kind}_{stem}": "rank" for kind in ("section", "kernel") for stem in ("tails", "onsets", "periods", "episodes")},
    "section_relative": "rank", "section_scores": "rank", "section_ratio": "rank", "section_z": "rank",
    **{name: "group" for name in ("section_reference", "kernel_reference", "section_floor", "kernel_floor", "section_fastest",
                                  "kernel_fastest", "ranks_with_data", "kernels", "section_columns")},
}


def _int_keyed(d):
    return isinstance(d, dict) and bool(d) and all(isinstance(k, int) for k in d)


def _kind(key, value):
    """What the integers of the mapping ``value`` under ``key`` are: a ``KEYED`` entry, a ``KEYED_BELOW`` entry + " below", or
    None where ``value`` has no integer keys (directly or one level down).  An unlisted mapping is refused."""
    if not isinstance(key, str) or not isinstance(value, dict):
        return None
    if _int_keyed(value):
        assert key in KEYED, f"full_report_script.KEYED does not say what the integer keys of {key!r} are: {sorted(value)[:8]}"
        return KEYED[key]
    if value and all(_int_keyed(sub) for sub in value.values()):
        assert key in KEYED_BELOW, f"full_report_script.KEYED_BELOW does not say what the integer keys below {key!r} are"
        return KEYED_BELOW[key] + " below"
    return None


def by_rank(value, group_of):
    """``value`` (a reader's nested dicts and lists) with every group label replaced by the sorted tuple of the group's ranks:
    what composed-with-labels and composed-with-inferred-groups can be compared by (the labels are 0 and 1, the roots 0 and
    ``ranks / 2``).  ``group_of``: ``{rank: label}`` of ALL ranks of the report ``value`` came from.  Not for
    ``work_groups()``, whose groups are named by their roots whatever the labels are."""
    members = {}
    for r, g in group_of.items():
        members.setdefault(g, []).append(r)
    names = {g: tuple(sorted(m)) for g, m in members.items()}

    def walk(v, key=None):
        if isinstance(v, dict):
            kind = _kind(key, v)
            if kind == "group":
                return {names[g]: walk(x) for g, x in v.items()}
            if kind == "rank to group":
                return {r: names[g] for r, g in v.items()}
            if kind == "group below":
                return {k: {names[g]: walk(x) for g, x in sub.items()} for k, sub in v.items()}
            if kind == "rank below":
                return {k: {r: walk(x) for r, x in sub.items()} for k, sub in v.items()}
            return {k: walk(x, k) for k, x in v.items()}
        if isinstance(v, list):
            return [walk(x) for x in v]
        return names[v] if key == "group" else v  # (a rank's record names its group)

    return walk(value)


def per_rank(value, ranks=None, path=()):
    """``{path: {rank: ...}}``: the mappings of a reader's result that ``KEYED`` / ``KEYED_BELOW`` say are keyed by rank, cut to
    ``ranks`` (None: all); mappings that are left empty are dropped, ``node_of`` (every rank, whatever the report covers) is
    left out.  What a rank's own report of a job that does not gather and the folded run's report can be compared by."""
    out = {}
    if not isinstance(value, dict):
        return out

    def cut(d):
        return {r: v for r, v in d.items() if ranks is None or r in ranks}

    for k, v in value.items():
        kind = _kind(k, v)
        if kind in ("rank", "rank to group"):
            if cut(v):
                out[path + (k,)] = cut(v)
        elif kind == "rank below":
            for name, sub in v.items():
                if cut(sub):
                    out[path + (k, name)] = cut(sub)
        elif kind is None:  # (no integer keys here: look further down; what is keyed by group, node or column holds no ranks)
            out.update(per_rank(v, ranks, path + (k,)))
    return out
