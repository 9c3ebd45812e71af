"""Slack scores for the CPU checker backend, and the NumPy restatement the slack tests compare against -- TEST
INFRASTRUCTURE, lives outside the product.

``slack_local_rows`` / ``slack_records`` restate the contract of include/nvrx_straggler.h (``nvrx_slack_local``,
``nvrx_slack_score``) in NumPy and plain Python: every sum is a SEQUENTIAL f64 sum in the contract's order (rows ascending,
columns ascending, kernel ids ascending), medians are taken by sorting keys -- nothing is shared with the kernels' wave
reductions and selections.  ``SlackOracleBackend`` / its rings are the checker with everything a report can carry
(``TrendOracleBackend``) plus ``slack_local`` / ``slack_list`` / ``slack_score`` built on it, so that the host side of the
feature runs on a box without a GPU.  ``CountingSlackBackend`` has slack methods that only count and raise: with the option
off nobody may call them.  ``scenario`` is the issue's sketch: 8 ranks, 200 calls of one collective per window.
"""
import numpy as np
import torch

from tail_oracle_backend import f2key
from trend_oracle_backend import TrendOracleBackend, TrendOracleRings, TrendOracleRingsFused

COLS = 64
NAN_BITS = np.uint32(0x7FC00000)
STAT_NUM, STAT_WEIGHT = 5, 6
GEMM = "gemm_kernel<bf16>"
ALLREDUCE = "ncclDevKernel_AllReduce_Sum_bf16_RING_LL(ncclDevKernelArgsStorage<4096ul>)"
RANKS, CALLS, SEED = 8, 200, 17


def scenario(late_rank=5, late_us=300.0, seed=SEED, ranks=RANKS, calls=CALLS, compute_us=1000.0):
    """``(step [calls], gemm [calls], in_collective [ranks, calls])`` f32 of one window: transfer 200 us +- 2 %, arrival skew
    exponential with mean 20 us, ``late_rank`` (None: nobody) arrives ``late_us`` late at every call.  The compute kernel
    and the step section are the same on every rank by construction."""
    rng = np.random.default_rng(seed)
    transfer = 200.0 * (1.0 + 0.02 * rng.standard_normal(calls))
    arrival = rng.exponential(20.0, (ranks, calls))
    if late_rank is not None:
        arrival[late_rank] += late_us
    last = arrival.max(0)
    coll = (transfer[None, :] + last[None, :] - arrival).astype(np.float32)
    return (compute_us + transfer + last).astype(np.float32), np.full(calls, compute_us, dtype=np.float32), coll


def play(be, late_rank=5, late_us=300.0, reports=1, stats_out=None, name_collectives=True, planned_out=None, **options):
    """The scenario through a gathering generator on the active backend ``be``, 8 logical ranks in one process, ``reports``
    identical windows.  Returns the reports, unread; ``stats_out`` (a list) takes every window's statistics rows, peeked
    just before its report.  ``name_collectives``: whether the caller's table of kernel rows names the all-reduce, as the
    Detector's does -- the generator then filters it into a new table at every report and every report takes the general,
    stepwise path; without it the second report on runs the cached plan (on the engine: the one-call report).  The slack
    step reads the rings' own table either way.  ``planned_out`` (a list) takes, per report, whether a planned one-call
    report has run by then."""
    from nvrx_straggler.reporting import ReportGenerator

    options.setdefault("collective_slack", True)
    gen = ReportGenerator(["relative_perf_scores"], gather_on_rank0=True, node_name="n", **options)
    rings = be.make_rings(RANKS, 4, 256)
    section_rows = {"step": rings.row_for(0, "step")}
    kernel_rows = {GEMM: rings.row_for(1, GEMM), ALLREDUCE: rings.row_for(1, ALLREDUCE)}
    passed_rows = kernel_rows if name_collectives else {GEMM: kernel_rows[GEMM]}
    step, gemm, coll = scenario(late_rank, late_us)
    out = []
    try:
        for _ in range(reports):
            for lr in range(RANKS):
                rings.push_many(section_rows["step"], step, lr=lr)
                rings.push_many(kernel_rows[GEMM], gemm, lr=lr)
                rings.push_many(kernel_rows[ALLREDUCE], coll[lr], lr=lr)
            if stats_out is not None:
                stats_out.append(np.array(rings.peek_stats(), dtype=np.float32))
            out.append(gen.generate_report_from_rings(rings, section_rows, passed_rows, local_ranks=RANKS))
            if planned_out is not None:
                planned_out.append(bool(gen._last_plan_fused))
            rings.reset()
    finally:
        gen.close()
    return out


def expected_scenario_records(stats, rows_per_rank=4, min_ranks=4):
    """The restatement's records of the scenario as ``play`` lays it out (rows: step, gemm, all-reduce), from the
    statistics rows ``stats`` [RANKS * rows_per_rank, 8] of that window as the engine under test computed them."""
    stats = np.asarray(stats, dtype=np.float32)
    slack = slack_local_rows(stats, [2], [column_of(ALLREDUCE)], 3, rows_per_rank, RANKS)
    table = np.zeros((RANKS, 2 * 2 + 1 + 1), dtype=np.float32)  # K = 1 (the gemm), S = 1 (the step)
    table[:, 0] = stats[1::rows_per_rank, 2]            # med of kernel id 0
    table[:, 4] = stats[1::rows_per_rank, STAT_WEIGHT]  # its weight
    return slack_records(slack, table, 1, 1, min_ranks)


def column_of(key):
    from nvrx_straggler.name_mapper import name_digest

    return name_digest(key) % COLS


def slack_local_rows(stats, rows, cols, rows_active, rows_per_rank, local_ranks):
    """``[local_ranks, 2, 64]`` f32 from the statistics rows ``stats`` [local_ranks * rows_per_rank, 8] and the (row, column)
    list (ascending rows): per (rank, column) one sequence of f64 additions in list order."""
    stats = np.asarray(stats, dtype=np.float32)
    out = np.zeros((local_ranks, 2, COLS), dtype=np.float32)
    out[:, 0, :] = -1.0
    active = rows_active or rows_per_rank
    assert list(rows) == sorted(set(rows))
    for q in range(local_ranks):
        t, n, seen = [0.0] * COLS, [0.0] * COLS, [False] * COLS
        for row, c in zip(rows, cols):
            if row >= active:
                continue
            num, weight = stats[q * rows_per_rank + row, STAT_NUM], stats[q * rows_per_rank + row, STAT_WEIGHT]
            if num >= 1:
                t[c] += float(weight)
                n[c] += float(num)
                seen[c] = True
        for c in range(COLS):
            if seen[c]:
                out[q, 0, c], out[q, 1, c] = np.float32(t[c]), np.float32(n[c])
    return out


def _lower_median_bits(values):
    """The bits of the element of rank (m - 1) >> 1 of the f32 ``values`` that are not NaN, in key order; NaN without one."""
    v = np.asarray(values, dtype=np.float32)
    v = v[~np.isnan(v)]
    if v.size == 0:
        return NAN_BITS
    order = np.argsort(f2key(v), kind="stable")
    return v[order[(v.size - 1) >> 1]].view(np.uint32)


def slack_records(slack, table, K, S, min_ranks):
    """``(job [8], columns [64, 4], ranks [R, 8])`` uint32 from the gathered rows ``slack`` [R, 2, 64] and the exchanged table
    [R, L] (``None`` at K = 0)."""
    slack = np.ascontiguousarray(slack, dtype=np.float32)
    R = slack.shape[0]
    assert slack.shape == (R, 2, COLS)
    min_ranks = min(min_ranks, R)
    t, n = slack[:, 0, :], slack[:, 1, :]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        present = (n > 0) & (t >= 0)
        avg = (t.astype(np.float64) / n.astype(np.float64)).astype(np.float32)
    cols = np.zeros((COLS, 4), dtype=np.uint32)
    floor = np.full(COLS, np.nan, dtype=np.float32)
    referenced = np.zeros(COLS, dtype=bool)
    for c in range(COLS):
        who = np.flatnonzero(present[:, c])
        cols[c, 1] = who.size
        referenced[c] = who.size >= min_ranks and who.size > 0
        if referenced[c]:
            a = avg[who, c]
            floor[c] = a[np.argmin(f2key(a))]
            cols[c, 0] = floor[c : c + 1].view(np.uint32)[0]
        else:
            cols[c, 0] = NAN_BITS
    ranks = np.zeros((R, 8), dtype=np.uint32)
    f = ranks.view(np.float32)
    KS = K + S
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for r in range(R):
            coll = waited = calls = 0.0
            columns = 0
            for c in range(COLS):
                if referenced[c] and present[r, c]:
                    coll += float(t[r, c])
                    waited += float(n[r, c]) * (float(avg[r, c]) - float(floor[c]))
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
    has = ranks[:, 5] > 0
    job = np.zeros(8, dtype=np.uint32)
    job[0] = _lower_median_bits(f[has, 1])
    job[1] = _lower_median_bits(f[has, 3])
    job[2] = int(has.sum())
    job[3] = int(referenced.sum())
    return job, cols, ranks


class _OracleSlack:
    def __init__(self, rec, first_rank, n_ranks):
        job, cols, ranks = rec
        self._rec = (job, cols, ranks[first_rank : first_rank + n_ranks])
        self.first_rank, self.n_ranks = first_rank, n_ranks
        self.reads = 0

    def records(self):
        self.reads += 1
        return self._rec


class _SlackRingsMixin:
    def slack_list(self):
        from nvrx_straggler.reporting import slack_row_list

        return slack_row_list(self.kernel_row_names)

    def slack_local(self, ws, rows_active=0, fused=False):
        be = self.backend
        be.slack_local_calls += 1
        rows, cols, _ = self.slack_list()
        be.slack_lists.append((tuple(rows), tuple(cols)))
        st, _ = self._stats()  # (the window the report just read: nothing was pushed or reset since)
        send, table = be.slack_buffers(ws)
        send.copy_(torch.from_numpy(slack_local_rows(st, rows, cols, rows_active, self.rows_per_rank, self.local_ranks)
                                    .reshape(self.local_ranks, 2 * COLS)))
        return send, table


class SlackOracleRings(_SlackRingsMixin, TrendOracleRings):
    pass


class SlackOracleRingsFused(_SlackRingsMixin, TrendOracleRingsFused):
    pass


class SlackOracleBackend(TrendOracleBackend):
    """The CPU checker with everything a report can carry, slack scores included (computed at enqueue time)."""

    name = "oracle-test+slack"

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.slack_local_calls = self.slack_score_calls = 0
        self.slack_lists, self.slack_args, self.slack_handles = [], [], []
        self._slack_bufs = {}

    def slack_buffers(self, ws):
        key = id(ws)
        if key not in self._slack_bufs:
            table = torch.zeros((ws.R, 2 * COLS), dtype=torch.float32)
            send = table if ws.R == ws.local_ranks else torch.zeros((ws.local_ranks, 2 * COLS), dtype=torch.float32)
            self._slack_bufs[key] = (send, table, ws)
        return self._slack_bufs[key][:2]

    def make_rings(self, local_ranks, rows_per_rank, ring_cap):
        cls = SlackOracleRingsFused if self.emulate_fused else SlackOracleRings
        return cls(self, local_ranks, rows_per_rank, ring_cap)

    def slack_score(self, ws, slack_table, table, first_rank=0, n_ranks=None, min_ranks=4):
        self.slack_score_calls += 1
        n_ranks = ws.R - first_rank if n_ranks is None else n_ranks
        self.slack_args.append((ws.R, ws.K, ws.S, first_rank, n_ranks, min_ranks))
        rec = slack_records(slack_table.numpy().reshape(ws.R, 2, COLS), table.numpy(), ws.K, ws.S, min_ranks)
        h = _OracleSlack(rec, first_rank, n_ranks)
        self.slack_handles.append(h)
        return h


class _RaisingSlackMixin:
    def slack_local(self, *a, **kw):
        self.backend.slack_calls += 1
        raise AssertionError("slack_local() called although collective_slack is off")

    def slack_list(self, *a, **kw):
        self.backend.slack_calls += 1
        raise AssertionError("slack_list() called although collective_slack is off")


class _RaisingSlackRings(_RaisingSlackMixin, TrendOracleRings):
    pass


class _RaisingSlackRingsFused(_RaisingSlackMixin, TrendOracleRingsFused):
    pass


class CountingSlackBackend(TrendOracleBackend):
    """The checker with everything else working and slack methods that only count and raise."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.slack_calls = 0

    def make_rings(self, local_ranks, rows_per_rank, ring_cap):
        cls = _RaisingSlackRingsFused if self.emulate_fused else _RaisingSlackRings
        return cls(self, local_ranks, rows_per_rank, ring_cap)

    def slack_score(self, *a, **kw):
        self.slack_calls += 1
        raise AssertionError("slack_score() called although collective_slack is off")


def named(found):
    """Ranks named anywhere in an ``identify_*stragglers`` result."""
    ranks = set()
    for v in found.values():
        for group in (v.values() if isinstance(v, dict) else [v]):
            ranks |= {s.rank for s in group}
    return sorted(ranks)
