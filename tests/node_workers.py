"""Worker functions and the scenario of the node-score tests (importable by spawned processes).  The CPU workers install the
checker backend WITH node scores themselves, as their first statement (``mp_util.run_ranks`` installs the plain one)."""
import pickle

import numpy as np

RANKS, PER_NODE, KERNELS, SAMPLES = 32, 8, 120, 200
SLOW_NODE, SLOW_RANK = 2, 5  # every rank of node 2 is 4 % slower in everything; rank 5 (node 0) is 4 % slower on its own
SEEDS = (0, 1, 2026)
KERNEL_NAMES = tuple(f"kernel_{k:03d}" for k in range(KERNELS))
SLOW_NODE_RANKS = list(range(SLOW_NODE * PER_NODE, (SLOW_NODE + 1) * PER_NODE))


def scenario_medians(seed=2026, ranks=RANKS, kernels=KERNELS, slow_node_factor=1.04, slow_members=PER_NODE):
    """``[ranks, kernels]`` f32 kernel medians in microseconds of a lockstep job on nodes of 8: lognormal kernel times (around
    100 us, sigma 0.5), 1 % noise per entry, the first ``slow_members`` ranks of node 2 ``slow_node_factor`` x slower in every
    kernel, and rank 5 on node 0 4 % slower on its own."""
    rng = np.random.default_rng(seed)
    base = rng.lognormal(np.log(100.0), 0.5, kernels)
    med = base[None, :] * (1.0 + 0.01 * rng.standard_normal((ranks, kernels)))
    med[SLOW_NODE * PER_NODE : SLOW_NODE * PER_NODE + slow_members] *= slow_node_factor
    med[SLOW_RANK] *= 1.04
    return med.astype(np.float32)


def ranks_named(ids):
    return sorted(getattr(s, "rank", s) for s in ids)


def _install_cpu_backend(**kw):
    from nvrx_straggler import backend
    from node_oracle_backend import NodeOracleBackend

    be = NodeOracleBackend(**kw)
    backend.set_backend(be)
    return be


def ring_reports_recorded(rank, world, gather_on_rank0, node_scores=True, emulate_fused=False, asynchronous=False,
                          node_groups=None):
    """Six ring reports on the checker backend with pace scores on and node scores on or off, the nodes taken from
    ``rank_to_node`` (two ranks per node name) unless ``node_groups`` says otherwise; a new section appears on the last rank at
    report 3 and a new kernel on rank 0 at report 5.  Returns the collectives this rank issued per report and what the
    reports said."""
    from tail_workers import record_collectives

    be = _install_cpu_backend(emulate_fused=emulate_fused)
    calls = record_collectives()
    from nvrx_straggler.reporting import ReportGenerator

    options = dict(node_scores=True, node_groups=node_groups, node_min_nodes=1) if node_scores else {}
    gen = ReportGenerator(["relative_perf_scores", "individual_perf_scores"], gather_on_rank0=gather_on_rank0,
                          node_name=f"host{rank // 2}", pace_scores=True, pace_min_ranks=2, asynchronous=asynchronous, **options)
    rings = be.make_rings(1, 16, 64)
    rng = np.random.default_rng(100 + rank)
    section_rows = {n: rings.row_for(0, n) for n in ("s0", "s1")}
    kernel_rows = {n: rings.row_for(1, n) for n in ("k0", "k1", "ncclDevKernel_z")}
    out, marks, fused, errors = [], [], [], []
    try:
        for i in range(6):
            if i == 2 and rank == world - 1:
                section_rows = dict(section_rows, s_new=rings.row_for(0, "s_new"))
            if i == 4 and rank == 0:
                kernel_rows = dict(kernel_rows, k_new=rings.row_for(1, "k_new"))
            for table in (section_rows, kernel_rows):
                for row in table.values():
                    rings.push_many(row, rng.lognormal(2.0 + 0.1 * rank, 0.3, 11 + 3 * i + rank).astype(np.float32))
            start = len(calls)
            planned = gen._ring_plan is not None  # (else this report takes the general path and plans the next ones)
            try:
                rep = gen.generate_report_from_rings(rings, section_rows, kernel_rows)
            except ValueError as e:  # (every collective of the report is behind it by then: the ranks stay in step)
                errors.append(str(e))
                rep = None
            rings.reset()
            marks.append(calls[start:])
            plan = gen._ring_plan
            fused.append(None if not planned or plan is None else bool(plan.fused))
            entry = {"node": None}
            if rep is not None:
                t = rep.node_scores()
                entry["node"] = t
                entry["pickled_same"] = repr(pickle.loads(pickle.dumps(rep)).node_scores()) == repr(t)
            out.append(entry)
        return {"calls": marks, "reports": out, "fused": fused, "node_calls": be.node_calls, "node_args": be.node_args,
                "errors": errors}
    finally:
        gen.close()


# ---- GPU workers (product backend) -------------------------------------------------------------------------------------
def _direct(be, ws, nodes, min_members, min_nodes):
    """What ``backend.node_score`` says of the workspace's table as it stands."""
    return be.node_score(ws, ws.table, nodes, 0, ws.R, min_members, min_nodes).records()


def folded_node(rank, world, reports=3, asynchronous=False):
    """The scenario through FoldedJob on the product backend (one section, the step, next to the 120 kernel rows; the nodes
    from ``node_groups="block:8"``): the general report, then planned ones.  Per report: what it said, whom the node rule and
    the pace rule name, the table it was computed from (read back from the workspace) and what ``backend.node_score`` says of
    that same table."""
    import torch

    from nvrx_straggler.backend import get_backend
    from nvrx_straggler.folded import FoldedJob

    torch.cuda.set_device(0)
    med = scenario_medians()
    job = FoldedJob(total_ranks=RANKS, section_names=["step"], ring_cap=256, scores_to_compute=("relative_perf_scores",),
                    node_name=f"node{rank}", kernel_names=KERNEL_NAMES, pace_scores=True, node_scores=True,
                    node_groups=f"block:{PER_NODE}", asynchronous=asynchronous)
    be = get_backend()
    try:
        out = []
        for i in range(reports):
            for lr, r in enumerate(job.logical_ranks()):
                job.load(lr, np.full((1, SAMPLES), med[r].sum(), dtype=np.float32))
                job.load_kernels(lr, np.repeat(med[r][:, None], SAMPLES, axis=1))
            rep = job.report()
            found = rep.identify_node_stragglers()
            entry = {"node": rep.node_scores(), "nodes_named": sorted(found["straggler_nodes"]),
                     "alone": ranks_named(found["ranks_off_pace_alone"]),
                     "pace_named": ranks_named(rep.identify_pace_stragglers()["straggler_gpus_relative"]),
                     "fused": getattr(job.reporter, "_last_plan_fused", None)}
            plan = job.reporter._ring_plan
            if plan is not None:
                ws = plan.ws
                be.synchronize()
                torch.cuda.synchronize()
                entry["shape"] = (ws.R, ws.K, ws.S)
                entry["table"] = ws.table.cpu().numpy().copy()
                nodes = job.reporter._node_for(ws)
                entry["nodes"] = (nodes.host.copy(), nodes.G, nodes.max_size)
                entry["direct"] = _direct(be, ws, nodes, 2, 3)
            out.append(entry)
        return out
    finally:
        job.close()


def folded_node_sync_then_async(rank, world, **options):
    """``folded_node`` twice in one process: synchronous reports, then asynchronous ones (each with rings of its own)."""
    return {"sync": folded_node(rank, world, asynchronous=False, **options),
            "async": folded_node(rank, world, asynchronous=True, **options)}


def folded_option_off(rank, world, reports=4, asynchronous=False):
    """Reports on the product backend with pace scores on and node scores OFF (``node_groups`` given all the same): the general
    report, then planned ones.  Returns what the real workspaces hold of the node step afterwards: the backend's workspaces
    that have a node buffer or a node step in flight and had neither before, the planned workspace's two fields, and what
    the generator resolved."""
    import torch

    from nvrx_straggler.backend import get_backend
    from nvrx_straggler.folded import FoldedJob

    torch.cuda.set_device(0)
    be = get_backend()

    def with_node_state():
        return [ws for ws in be._workspaces.values() if ws._table_state and "node" in ws._table_state]

    before = with_node_state()  # (other jobs of this process may have left theirs; the objects are kept alive, so ids hold)
    job = FoldedJob(total_ranks=6, section_names=["step"], ring_cap=64, scores_to_compute=("relative_perf_scores",),
                    kernel_names=("gemm", "copy"), pace_scores=True, pace_min_ranks=2, node_groups="block:2",
                    asynchronous=asynchronous)
    try:
        said, fused = [], []
        for w in range(reports):
            for lr in range(6):
                job.load(lr, np.full((1, 9), 100.0 * (w + 1) + lr, dtype=np.float32))
                job.load_kernels(lr, np.full((2, 9), 10.0 * (w + 1) + lr, dtype=np.float32))
            rep = job.report()
            said.append((rep.node_scores(), bool(rep.pace_scores()), "_node" in rep.__dict__))
            fused.append(getattr(job.reporter, "_last_plan_fused", None))
        be.synchronize()
        torch.cuda.synchronize()
        ws = job.reporter._ring_plan.ws
        slots = ws._table_state or {}  # slot -> its buffer and the step in flight, for the slots that ever ran
        node = slots.get("node")
        assert set(slots) == {"pace"}, sorted(slots)  # (robust and peer scores are off as well; pace scores ran)
        return {"said": said, "fused": fused, "new": [w for w in with_node_state() if not any(w is b for b in before)],
                "planned_ws": (node and node.buf, node and node.last, "node" in slots, (ws.R, ws.K, ws.S)),
                "resolved": job.reporter._node_resolved, "option": job.reporter.node_scores}
    finally:
        job.close()


def held_reports(rank, world, windows=5):
    """Reports held across the next two on the same workspace: every window's kernel takes another time, and each report is
    read only after two more were issued.  Four ranks on two nodes (``mod:2``: {0, 2} and {1, 3})."""
    import torch

    from nvrx_straggler.folded import FoldedJob

    torch.cuda.set_device(0)
    job = FoldedJob(total_ranks=4, section_names=["step"], ring_cap=64, scores_to_compute=("relative_perf_scores",),
                    kernel_names=("gemm",), node_scores=True, node_groups="mod:2", node_min_nodes=1)
    try:
        held, out = [], []
        for w in range(windows):
            for lr in range(4):
                job.load(lr, np.full((1, 9), 100.0 * (w + 1) + lr, dtype=np.float32))
                job.load_kernels(lr, np.full((1, 9), 10.0 * (w + 1) + lr, dtype=np.float32))
            held.append(job.report())
            if w >= 2:
                out.append(held[w - 2].node_scores())
        out.extend(h.node_scores() for h in held[-2:])
        return out
    finally:
        job.close()


def detector_rehomed(rank, world, windows=12, sections=3):
    """Asynchronous Detector reports with node scores (one rank, one node from ``rank_to_node``, both thresholds 1), re-homed
    onto the stream their stamps ran on (forced by a 1 us gap): section i of window t holds samples of 10 t + i only, so a node
    step that read another window's table would show another center.  Per report: what it said, the table it was computed
    from and what ``backend.node_score`` says of that same table."""
    import torch

    from nvrx_straggler import Detector
    from nvrx_straggler.backend import get_backend

    Detector.initialize(scores_to_compute="all", gather_on_rank0=True, node_name="n", asynchronous=True, node_scores=True,
                        node_min_members=1, node_min_nodes=1)
    try:
        names = [f"s{i}" for i in range(sections)]
        for name in names:
            with Detector.detection_section(name, profile_cuda=True):
                pass
        Detector.generate_report()
        rings, be = Detector.rings, get_backend()
        secs = [Detector.custom_sections[name] for name in names]
        gpu_rows = [rings.kernel_row_names[f"hipevent::{name}"] for name in names]
        big = torch.randn(4096, 4096, device="cuda")
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        torch.cuda.synchronize()
        out = []
        for t in range(1, windows + 1):
            st = streams[t % 2]
            with torch.cuda.stream(st):
                (big @ big).sum()  # the report of this window queues behind it on this stream
                for i, (sec, gpu_row) in enumerate(zip(secs, gpu_rows)):
                    for _ in range(3):
                        rings.stamp_begin(gpu_row, st.cuda_stream)
                        rings.stamp_end(gpu_row, st.cuda_stream, sec.row, float(10 * t + i))
                rep = Detector.generate_report()  # returns at once; re-homed onto `st`
            torch.cuda.synchronize()
            be.synchronize()
            entry = {"node": rep.node_scores()}
            plan = Detector.reporter._ring_plan
            if plan is not None:
                ws = plan.ws
                entry["shape"] = (ws.R, ws.K, ws.S)
                entry["table"] = ws.table.cpu().numpy().copy()
                nodes = Detector.reporter._node_for(ws)
                entry["nodes"] = (nodes.host.copy(), nodes.G, nodes.max_size)
                entry["direct"] = _direct(be, ws, nodes, 1, 1)
                be.synchronize()
            out.append(entry)
        return {"reports": out, "rehomed": int(rings.lib.nvrx_ctx_info(rings.ctx, 5)), "lane_is_none": Detector._lane is None}
    finally:
        Detector.shutdown()
