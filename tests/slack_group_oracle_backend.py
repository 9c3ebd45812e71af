"""Slack scores per peer group for the CPU checker backend, and the NumPy restatement the tests compare against -- TEST
INFRASTRUCTURE, lives outside the product.

``slack_group_records`` restates the contract of include/nvrx_straggler.h (``nvrx_slack_group_score``) in NumPy and plain
Python, the guards of hostile ``d_groups`` contents included: every sum is a SEQUENTIAL f64 sum in ascending column order,
floors and medians are taken by sorting keys -- nothing is shared with the kernels' wave reductions and selections, and nothing
reads their output.  ``SlackGroupOracleBackend`` is ``PeerHistoryOracleBackend`` plus
``slack_group_score`` (it lacks the four ``*_group_score`` methods of the row families: the checker that serves a report with
every option on is tests/full_oracle_backend.py's ``FullOracleBackend``); ``CountingSlackGroupBackend`` has a grouped method that only counts and raises: with the option off
nobody may call it.  ``stage_scenario`` / ``play_stages`` are the issue's sketch: 8 ranks in two pipeline stages, a
stage-local all-reduce and a send / receive bubble that differs per stage.
"""
import numpy as np

from peer_history_oracle_backend import PeerHistoryOracleBackend
from slack_oracle_backend import COLS, NAN_BITS, _OracleSlack, _lower_median_bits
from tail_oracle_backend import f2key

RANKS, CALLS, SEED = 8, 200, 17
ALLREDUCE = "ncclDevKernel_AllReduce_Sum_bf16_RING_LL(ncclDevKernelArgsStorage<4096ul>)"
SENDRECV = "ncclDevKernel_SendRecv(ncclDevKernelArgsStorage<4096ul>)"
STAGE_GEMMS = ("gemm_stage0<bf16>", "gemm_stage1<bf16>")
BUBBLE_US = (60.0, 420.0)
TWO_SIX = (0, 0, 1, 1, 1, 1, 1, 1)
FOUR_FOUR = (0, 0, 0, 0, 1, 1, 1, 1)


def groups_array(labels):
    """``group[R] | members[R] | start[G+1]`` int32 of dense group ids ``labels``, and G."""
    group = np.asarray(labels, dtype=np.int32)
    G = int(group.max()) + 1
    members = np.argsort(group, kind="stable").astype(np.int32)
    start = np.zeros(G + 1, dtype=np.int32)
    np.cumsum(np.bincount(group, minlength=G), out=start[1:])
    return np.concatenate((group, members, start)), G


def slack_group_records(slack, table, K, S, groups_host, G, max_group, min_ranks, min_peers):
    """``(groups [G, 8], pairs [G, 64, 4], ranks [R, 8])`` uint32 from the gathered rows ``slack`` [R, 2, 64], the exchanged
    table [R, L] (``None`` at K = 0) and the array ``groups_host`` as the device would see it, whatever it holds."""
    slack = np.ascontiguousarray(slack, dtype=np.float32)
    R = slack.shape[0]
    assert slack.shape == (R, 2, COLS)
    gh = np.asarray(groups_host, dtype=np.int64)
    assert gh.size == 2 * R + G + 1
    group, members, start = gh[:R], gh[R : 2 * R], gh[2 * R :]
    t, n = slack[:, 0, :], slack[:, 1, :]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        present = (n > 0) & (t >= 0)
        avg = (t.astype(np.float64) / n.astype(np.float64)).astype(np.float32)
    keys = f2key(avg)

    # the stretches: starts clamped to [0, R], never negative in length, cut to max_group; entries outside [0, R) skipped
    stretch, sizes = [], []
    for g in range(G):
        s0, s1 = min(max(int(start[g]), 0), R), min(max(int(start[g + 1]), 0), R)
        size = min(max(s1 - s0, 0), max_group)
        sizes.append(size)
        stretch.append([int(m) for m in members[s0 : s0 + size] if 0 <= m < R])

    pairs = np.zeros((G, COLS, 4), dtype=np.uint32)
    floor = np.full((G, COLS), np.nan, dtype=np.float32)
    referenced = np.zeros((G, COLS), dtype=bool)
    for g in range(G):
        need = max(min_peers, min(min_ranks, sizes[g]))
        idx = np.asarray(stretch[g], dtype=np.int64)
        # (key, rank) as one sortable word per (member, column); absent entries above every present one
        order = (keys[idx].astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)[:, None]
        order[~present[idx]] = np.uint64(0xFFFFFFFFFFFFFFFF)
        for c in range(COLS):
            count = int(present[idx, c].sum())
            pairs[g, c, 1], pairs[g, c, 3] = count, sizes[g]
            if count >= need:
                best = int(order[:, c].min() & np.uint64(0xFFFFFFFF))
                referenced[g, c] = True
                floor[g, c] = avg[best, c]
                pairs[g, c, 0] = avg[best : best + 1, c].view(np.uint32)[0]
                pairs[g, c, 2] = best
            else:
                pairs[g, c, 0], pairs[g, c, 2] = NAN_BITS, 0xFFFFFFFF

    ranks = np.zeros((R, 8), dtype=np.uint32)
    f = ranks.view(np.float32)
    KS = K + S
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for r in range(R):
            g = int(group[r]) if 0 <= group[r] < G else -1
            coll = waited = calls = 0.0
            columns = 0
            for c in range(COLS):
                if g >= 0 and referenced[g, c] and present[r, c]:
                    coll += float(t[r, c])
                    waited += float(n[r, c]) * (float(avg[r, c]) - float(floor[g, c]))
                    calls += float(n[r, c])
                    columns += 1
            comp = 0.0
            for k in range(K):
                if table[r, k] >= 0:
                    comp += float(table[r, 2 * KS + k])
            if columns:
                f[r, 0], f[r, 1], f[r, 2] = np.float32(coll), np.float32(waited), np.float32(comp)
                f[r, 3] = np.float32(np.float64(waited) / (np.float64(coll) + np.float64(comp)))
                ranks[r, 4] = 0xFFFFFFFF if calls >= 4294967295.0 else (int(calls) if calls >= 0 else 0)
                ranks[r, 5] = columns
            else:
                ranks[r, :4] = NAN_BITS
            ranks[r, 6] = int(present[r].sum())
            ranks[r, 7] = np.int64(g) & 0xFFFFFFFF

    groups = np.zeros((G, 8), dtype=np.uint32)
    for g in range(G):
        with_data = [m for m in stretch[g] if ranks[m, 5] > 0]
        groups[g, 0] = _lower_median_bits(f[with_data, 1])
        groups[g, 1] = _lower_median_bits(f[with_data, 3])
        groups[g, 2] = len(with_data)
        groups[g, 3] = int(referenced[g].sum())
        groups[g, 4] = sizes[g]
    return groups, pairs, ranks


class _OracleSlackGroup(_OracleSlack):
    def __init__(self, rec, G, first_rank, n_ranks):
        super().__init__(rec, first_rank, n_ranks)
        self.G = G


class SlackGroupOracleBackend(PeerHistoryOracleBackend):
    """The CPU checker up to the peer-score history plus the slack scores per peer group (computed at enqueue time).  It
    lacks the row families' ``*_group_score`` methods: a report with ``row_peer_groups`` too needs
    ``full_oracle_backend.FullOracleBackend``."""

    name = "oracle-test+slack-group"

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.slack_group_calls = 0
        self.slack_group_args, self.slack_group_handles = [], []

    def slack_group_score(self, ws, slack_table, table, groups, first_rank=0, n_ranks=None, min_ranks=4, min_peers=2):
        self.slack_group_calls += 1
        n_ranks = ws.R - first_rank if n_ranks is None else n_ranks
        self.slack_group_args.append((ws.R, ws.K, ws.S, groups.G, groups.max_size, first_rank, n_ranks, min_ranks, min_peers))
        rec = slack_group_records(slack_table.numpy().reshape(ws.R, 2, COLS), table.numpy(), ws.K, ws.S, groups.host, groups.G,
                                  groups.max_size, min_ranks, min_peers)
        h = _OracleSlackGroup(rec, groups.G, first_rank, n_ranks)
        self.slack_group_handles.append(h)
        return h


class CountingSlackGroupBackend(PeerHistoryOracleBackend):
    """The checker with everything else working -- the job-wide slack scores and the peer scores included -- and a grouped
    slack method that only counts and raises."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.slack_group_calls = 0

    def slack_group_score(self, *a, **kw):
        self.slack_group_calls += 1
        raise AssertionError("slack_group_score() called although slack_peer_groups is off")


def stage_scenario(labels=TWO_SIX, late_rank=5, late_us=300.0, seed=SEED, calls=CALLS, compute_us=1000.0):
    """``(step [ranks, calls], gemm [calls], allreduce [ranks, calls], bubble [ranks, calls])`` f32 of one window of a
    two-stage pipeline job, ``labels`` being the stage of each rank.  The all-reduce is stage-local: transfer 200 us +- 2 %,
    arrival skew exponential with mean 20 us, a rank's time is the transfer plus the wait for the latest arrival IN ITS
    STAGE; ``late_rank`` (None: nobody) arrives ``late_us`` late at every call.  The bubble is 60 us in stage 0 and 420 us in
    stage 1, +- 2 %.  The draws come in that order: transfer, arrival, bubble noise."""
    stage = np.asarray(labels)
    ranks = stage.size
    rng = np.random.default_rng(seed)
    transfer = 200.0 * (1.0 + 0.02 * rng.standard_normal(calls))
    arrival = rng.exponential(20.0, (ranks, calls))
    noise = rng.standard_normal((ranks, calls))
    if late_rank is not None:
        arrival[late_rank] += late_us
    last = np.stack([arrival[stage == stage[r]].max(0) for r in range(ranks)])
    allreduce = transfer[None, :] + last - arrival
    bubble = np.asarray(BUBBLE_US)[stage][:, None] * (1.0 + 0.02 * noise)
    step = compute_us + allreduce + bubble
    return (step.astype(np.float32), np.full(calls, compute_us, dtype=np.float32), allreduce.astype(np.float32),
            bubble.astype(np.float32))


def play_stages(be, labels=TWO_SIX, late_rank=5, reports=1, local_ranks=RANKS, lr0=0, stats_out=None, planned_out=None,
                **options):
    """The stage scenario through a generator on the active backend ``be``: ``local_ranks`` logical ranks from ``lr0`` on in
    this process, ``reports`` identical windows.  Each stage runs its own GEMM (what ``peer_groups="auto"`` tells the stages
    apart by); the caller's table of kernel rows names the compute kernels only, as in ``slack_oracle_backend.play`` with
    ``name_collectives=False``: the first report is stepwise, later ones run the cached plan.  Returns the reports, unread."""
    from nvrx_straggler.reporting import ReportGenerator

    options.setdefault("collective_slack", True)
    options.setdefault("gather_on_rank0", True)
    gen = ReportGenerator(["relative_perf_scores"], node_name="n", **options)
    rings = be.make_rings(local_ranks, 8, 256)
    section_rows = {"step": rings.row_for(0, "step")}
    kernel_rows = {k: rings.row_for(1, k) for k in STAGE_GEMMS + (ALLREDUCE, SENDRECV)}
    passed_rows = {k: kernel_rows[k] for k in STAGE_GEMMS}
    step, gemm, allreduce, bubble = stage_scenario(labels, late_rank)
    out = []
    try:
        for _ in range(reports):
            for lr in range(local_ranks):
                r = lr0 + lr
                rings.push_many(section_rows["step"], step[r], lr=lr)
                rings.push_many(kernel_rows[STAGE_GEMMS[labels[r]]], gemm, lr=lr)
                rings.push_many(kernel_rows[ALLREDUCE], allreduce[r], lr=lr)
                rings.push_many(kernel_rows[SENDRECV], bubble[r], lr=lr)
            if stats_out is not None:
                stats_out.append(np.array(rings.peek_stats(), dtype=np.float32))
            out.append(gen.generate_report_from_rings(rings, section_rows, passed_rows, local_ranks=local_ranks))
            if planned_out is not None:
                planned_out.append(bool(gen._last_plan_fused))
            rings.reset()
    finally:
        gen.close()
    return out
