#!/usr/bin/env python3
"""Straggler detection on MI355X in a small data-parallel training loop.

What the reference's ``examples/straggler/example.py`` shows on CUDA, on ROCm: every rank wraps its forward pass in
``Detector.detection_section("fwd", profile_cuda=True)``, all ranks call ``Detector.generate_report()`` every
``--report-interval`` steps, rank 0 prints the relative and individual GPU scores and whoever ``identify_stragglers``
flags, with the ROCm SMI telemetry line of this rank's GPU next to it.  The data is synthetic (MNIST-shaped): there is
nothing to download.

    # one process per GPU over RCCL (the package is imported before torch touches the GPU: in a multi-rank job that
    # selects per-kernel GPU timing, the reference's data model -- collectives inside the section do not hide a slow GPU)
    python examples/straggler_example.py --num-processes 8

    # a box with ONE GPU: the ranks share it over gloo
    python examples/straggler_example.py --num-processes 2 --share-gpu

To see a straggler, slow one GPU down while it runs -- the ROCm counterpart of the reference's ``nvidia-smi -lgc 800``:

    rocm-smi -d 3 --setperflevel low          # ... and `--setperflevel auto` to give it back

or let the example do it: ``--slow-rank 3`` holds that rank's shader clock at its lowest level through ROCm SMI from
step ``--slow-from`` on (root and a writable sysfs needed).  Where the driver refuses, or on a box whose ranks share one
GPU, ``--slow-by simulated`` puts a stand-in for "a kernel that takes longer on a slower GPU" into every rank's section:
a spin kernel whose duration is its argument, 1.5x longer on the slow rank -- the report then reads as it would with a
GPU at two thirds of its speed.

With ``NVRX_KERNEL_ATTRIBUTION=5`` in the environment the report also names, for every flagged rank, the five kernels that
carry most of its score's deficit (``Report.explain_gpu_scores()``).

A GPU that is slow only SOME of the time does not move a median: ``--slow-by intermittent`` applies the simulated slowdown
on every ``--slow-every``-th step of the slow rank only, and the lines above stay quiet.  With ``NVRX_TAIL_QUANTILE=0.9`` in
the environment the report also compares the 0.9 quantile of every timing row across ranks (``Report.tail_scores()``) and
the example prints whoever ``identify_tail_stragglers`` flags underneath.

With ``NVRX_ROBUST_SCORES=1`` the report also rates every rank against the job's median and spread
(``Report.robust_scores()``) and the example prints each GPU's z-score and whoever ``identify_robust_stragglers`` flags.

A GPU that BECOMES slow late in a window does not move a median either: ``--slow-by onset`` makes the slow rank's stand-in
kernel 1.5x longer from 70 % of every report window on.  With ``NVRX_ONSET_DETECTION=1`` the report also looks for the one
step in every timing row that explains most of its variance (``Report.onset_scores()``) and the example prints whoever
``identify_onset_stragglers`` flags, with how many samples ago the rank's largest shift happened.

``--slow-by intermittent --slow-every N`` is also a BEAT: the slow rank stalls on every N-th step.  With
``NVRX_PERIOD_DETECTION=1`` the report folds every timing row over every period up to a quarter of its samples
(``Report.period_scores()``) and the example prints whoever ``identify_period_stragglers`` flags, with the period of the
rank's largest excess and how many samples ago its slow phase last occurred.

``--slow-by stretch`` makes the slow rank's GPU kernel 1.5x longer for ONE stretch of every report window (from 60 % to 70 %
of it) and normal again afterwards: no median, no 0.95-quantile, no step and no beat shows it.  With
``NVRX_EPISODE_DETECTION=1`` the report also looks for the one interval of every timing row that spent most time above the
row's mean (``Report.episode_scores()``) and the example prints whoever ``identify_episode_stragglers`` flags, with how long
the rank's strongest episode lasted and how many samples ago it ended.

``--persist`` needs no training loop: it plays 20 reports of a job of 8 ranks (folded onto one GPU, 1 % noise, seed 17) in which
rank 2 is 1.6x slower in report 6 only and rank 5 is 1.45x slower from report 10 on, with a score history of 8 reports
(``ReportGenerator(score_history=8, persistence_min_reports=3)``), and prints per report whom ``identify_stragglers`` flags and
whom ``identify_persistent_stragglers`` does: rank 2 once and never persistently, rank 5 from report 10 and, persistently,
from report 12 on.

``--trend`` needs no training loop either: it plays 48 reports of a job of 8 ranks (folded onto one GPU, 1 % noise, seed 23) in
which rank 5 gets 1.2 % slower with every report from report 8 on and rank 2 is 1.4x slower in report 14 only, with a score
history of 16 reports and score trends (``ReportGenerator(score_history=16, persistence_min_reports=3, score_trends=True)``),
and prints per report whom ``identify_declining_stragglers`` names next to the two rules above, with rank 5's slope, level and
``reports_left``; at the end, the first report at which each rule named rank 5.

``--slack`` needs no training loop either: it plays one report window of a job of 8 ranks (folded onto one GPU, seed 17) that
runs 200 steps of one compute kernel (1000 us) and one all-reduce (200 us +- 2 % of transfer; the ranks arrive with an
exponential skew of 20 us) in which rank 5's HOST is slow: it arrives 300 us late at every collective.  Its kernels take the
usual time and the step lasts as long on every rank, so ``identify_stragglers`` names nobody; with slack scores
(``ReportGenerator(collective_slack=True)``) ``identify_slack_stragglers`` names rank 5, and the report says what it costs.

``--peer`` needs no training loop either: it plays one report of a job of 8 ranks in two pipeline stages (folded onto one GPU,
1 % noise, seed 29): ranks 0-3 run a stage of 1000 us, ranks 4-7 one of 1500 us, and rank 6 is 1.4x slower than its stage's
peers.  ``identify_stragglers`` names ranks 4-7, three of them healthy; with peer groups (``ReportGenerator(peer_groups=
"block:4")``) ``identify_peer_stragglers`` names rank 6 alone, and both scores are printed side by side.

``--peer-persist`` plays the ``--peer`` job over 16 reports (8 ranks, ``block:4``, stages of 1000 us and 1500 us, 1 % noise, seed
37): rank 1 is 1.6x slower in report 6 only, rank 6 is 1.4x slower than its stage from report 10 on.  Per report it prints whom
each rule names.  Per-report peer flagging (``identify_peer_stragglers``) names rank 1 at report 6 -- with ``stop_if_detected``
one bad window would end the job -- and rank 6 from report 10; the job-wide history (``identify_persistent_stragglers``) names
the healthy ranks 4-7 from the third report on, for ever; the peer history (``ReportGenerator(peer_history=8,
peer_persistence_min_reports=3)``, ``identify_persistent_peer_stragglers``) never names rank 1 and names rank 6 alone from
report 12 on.

``--pace`` needs no training loop either: it plays one report of a job of 8 ranks x 120 kernels (folded onto one GPU, lognormal
kernel times, 1 % noise per entry, seed 2026, 200 calls of every kernel) in which rank 5 is 4 % slower in EVERY kernel -- a card
held a clock step down.  Its relative GPU score reads about 0.95 and its robust z about 2: ``identify_stragglers`` and
``identify_robust_stragglers`` name nobody; with pace scores (``ReportGenerator(pace_scores=True)``) the report says that rank
5 is slower than the job's median in 120 of 120 kernels, and ``identify_pace_stragglers`` names it alone.

``--pace-peer`` plays the same kind of report for a PIPELINE job: 8 ranks x 120 kernels in two stages (``block:4``), the second
stage 1.5 x slower in every kernel, and rank 6 4 % slower than its stage in every kernel.  Against the median of the whole job
every rank of the slower stage is slower in 120 of 120 kernels and ``identify_pace_stragglers`` names ranks 4-7, three of them
healthy; with ``ReportGenerator(pace_peer_groups=True)`` each rank is rated against the median of its own stage and rank 6 is
named alone.  Both are printed.

``--node`` plays a report of 32 ranks x 120 kernels on 4 nodes of 8 (``node_groups="block:8"``; 1 % noise, seed 2026) in which
every rank of node 2 is 4 % slower in every kernel -- failed fans, a capped PSU -- and rank 5 on node 0 is 4 % slower on its
own.  ``identify_pace_stragglers`` names nine ranks and cannot say which of them are one incident; with node scores
(``ReportGenerator(node_scores=True)``) ``identify_node_stragglers`` names node 2 alone, 8 of its 8 ranks agreeing, and hands
rank 5 back as a rank that is off pace without its node.

``--work`` plays the ``--peer`` job WITHOUT anybody describing its layout: 8 ranks in two pipeline stages (folded onto one GPU,
1 % noise, seed 31), 120 kernel keys and 4 sections; 100 keys are shared and run 1600 times a window in stage 0 and 2400 times
in stage 1, 10 keys only stage 0 has and 10 only stage 1; rank 6 is 1.4x slower in everything.  ``identify_stragglers`` names
ranks 4-7; with ``ReportGenerator(peer_groups="auto")`` the groups are inferred from the table the report gathers anyway --
which kernels a rank has and how often each ran, neither of which a slow GPU changes --, ``identify_peer_stragglers`` names
rank 6 alone, and the inferred groups are printed with every rank's nearest other rank.
"""
import argparse
import os
import socket
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "nvidia-resiliency-ext_amd")]

# the drop-in import path of the reference package; importing it BEFORE the HIP runtime starts lets a multi-rank job use
# per-kernel GPU timing (rocprofiler-sdk accepts tools only before that)
from nvidia_resiliency_ext.attribution import straggler  # noqa: E402

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402
import torch.nn as nn  # noqa: E402
from torch.nn.parallel import DistributedDataParallel as DDP  # noqa: E402


class Model(nn.Module):
    def __init__(self, width: int):
        super().__init__()
        self.layers = nn.Sequential(nn.Linear(784, width), nn.ReLU(), nn.Linear(width, width), nn.ReLU(), nn.Linear(width, width),
                                    nn.ReLU(), nn.Linear(width, 10))

    def forward(self, x):
        return self.layers(torch.flatten(x, 1))


def train(args) -> None:
    # the order of the reference's example (examples/straggler/example.py:60-66): the detector first, the GPU afterwards --
    # the detector's device side is created at the first section, on the device that is current then
    straggler.Detector.initialize(gather_on_rank0=True)
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    device_index = 0 if args.share_gpu else local_rank
    if world > 1:
        dist.init_process_group("gloo" if args.share_gpu else "nccl")
    torch.cuda.set_device(device_index)
    device = torch.device("cuda", device_index)
    torch.manual_seed(42 + rank)
    model = Model(args.width).to(device)
    net = DDP(model, device_ids=None if args.share_gpu else [device_index]) if world > 1 else model
    optim = torch.optim.SGD(net.parameters(), lr=0.01, momentum=0.5)
    loss_fn = nn.CrossEntropyLoss()
    data = torch.randn(args.batch_size, 1, 28, 28, device=device)
    target = torch.randint(0, 10, (args.batch_size,), device=device)
    slow_ctx = None
    t_start = time.monotonic()
    for step in range(args.steps):
        if rank == args.slow_rank and step == args.slow_from and args.slow_by == "clock":
            from nvrx_straggler import gpu_telemetry

            try:
                slow_ctx = gpu_telemetry.slowed_down(device_index).__enter__()
                print(f"[rank {rank}] shader clock of GPU {device_index} held at its lowest level from step {step} on", flush=True)
            except gpu_telemetry.SmiRefused as e:
                print(f"[rank {rank}] ROCm SMI refused to slow the GPU down ({e}); use --slow-by simulated", flush=True)
        with straggler.Detector.detection_section("fwd", profile_cuda=True):
            output = net(data)
            if args.slow_by in ("simulated", "intermittent", "onset", "stretch"):   # one kernel whose duration says how fast "this GPU" is
                slow = rank == args.slow_rank and step >= args.slow_from
                if args.slow_by == "intermittent":
                    slow = slow and step % args.slow_every == 0
                if args.slow_by == "onset":  # (a window: the steps behind one report up to and including the next one's)
                    slow = slow and (step - 1) % args.report_interval >= 0.7 * args.report_interval
                if args.slow_by == "stretch":  # (one stretch of every window, and normal again behind it)
                    slow = slow and 0.6 * args.report_interval <= (step - 1) % args.report_interval < 0.7 * args.report_interval
                torch.cuda._sleep(int(args.simulated_cycles * (1.5 if slow else 1.0)))
        loss = loss_fn(output, target)
        optim.zero_grad()
        loss.backward()
        optim.step()
        if step % args.report_interval == 0 and step:
            report = straggler.Detector.generate_report()
            if rank == 0:
                print(f"step {step}: GPUs relative perf: { {r: round(s, 3) for r, s in report.gpu_relative_perf_scores.items()} }")
                print(f"step {step}: GPUs individual perf: { {r: round(s, 3) for r, s in report.gpu_individual_perf_scores.items()} }")
                found = report.identify_stragglers(gpu_rel_threshold=args.threshold, gpu_indiv_threshold=args.threshold)
                explained = report.explain_gpu_scores()  # {} unless NVRX_KERNEL_ATTRIBUTION=N asks for the top-N kernels
                for kind, family in (("straggler_gpus_relative", "relative"), ("straggler_gpus_individual", "individual")):
                    if found[kind]:
                        print(f"step {step}: {kind}: {sorted((s.rank, s.node) for s in found[kind])}")
                    for s in sorted(found[kind], key=lambda s: s.rank):
                        why = explained.get(family, {}).get(s.rank)
                        if why:
                            print(f"step {step}:   rank {s.rank}: {why['deficit']:.3f} of its {family} score is missing, "
                                  f"{why['explained']:.3f} of it in:")
                            for k in why["kernels"]:
                                print(f"step {step}:     {k['kernel']}: share {k['share']:.3f}, score {k['score']:.3f}, "
                                      f"{k['lost_us']:.0f} us above the reference pace")
                tails = report.tail_scores()  # {} unless NVRX_TAIL_QUANTILE=q asks for tail scores
                if tails:
                    print(f"step {step}: GPUs relative tail perf (q={tails['quantile']:g}): "
                          f"{ {r: round(s, 3) for r, s in tails['gpu_relative'].items()} }")
                    tail_found = report.identify_tail_stragglers(gpu_rel_threshold=args.threshold)
                    if tail_found["straggler_gpus_relative"]:
                        print(f"step {step}: tail straggler_gpus_relative: "
                              f"{sorted((s.rank, s.node) for s in tail_found['straggler_gpus_relative'])}")
                robust = report.robust_scores()  # {} unless NVRX_ROBUST_SCORES=1 asks for robust scores
                if robust:
                    print(f"step {step}: GPUs z against the job's median: { {r: round(z, 2) for r, z in robust['gpu_z'].items()} }")
                    robust_found = report.identify_robust_stragglers()
                    if robust_found["straggler_gpus_relative"]:
                        print(f"step {step}: robust straggler_gpus_relative: "
                              f"{sorted((s.rank, s.node) for s in robust_found['straggler_gpus_relative'])}")
                onsets = report.onset_scores()  # {} unless NVRX_ONSET_DETECTION=1 asks for onset scores
                if onsets:
                    print(f"step {step}: GPUs relative onset perf: { {r: round(s, 3) for r, s in onsets['gpu_relative'].items()} }")
                    onset_found = report.identify_onset_stragglers(gpu_rel_threshold=args.threshold)
                    if onset_found["straggler_gpus_relative"]:
                        print(f"step {step}: onset straggler_gpus_relative: "
                              f"{sorted((s.rank, s.node) for s in onset_found['straggler_gpus_relative'])}")
                    for s in sorted(onset_found["straggler_gpus_relative"], key=lambda s: s.rank):
                        rows = [(per[s.rank], name) for name, per in onsets["kernel_onsets"].items() if s.rank in per]
                        if rows:
                            rec, name = max(rows, key=lambda x: x[0]["shift"])
                            print(f"step {step}:   rank {s.rank}: {name} became {rec['shift']:.2f}x slower {rec['samples_ago']} "
                                  f"samples ago (of {rec['window']}; the step explains {rec['strength']:.2f} of the row's variance)")
                periods = report.period_scores()  # {} unless NVRX_PERIOD_DETECTION=1 asks for period scores
                if periods:
                    print(f"step {step}: GPUs relative period perf: { {r: round(s, 3) for r, s in periods['gpu_relative'].items()} }")
                    period_found = report.identify_period_stragglers(gpu_rel_threshold=args.threshold)
                    if period_found["straggler_gpus_relative"]:
                        print(f"step {step}: period straggler_gpus_relative: "
                              f"{sorted((s.rank, s.node) for s in period_found['straggler_gpus_relative'])}")
                    for s in sorted(period_found["straggler_gpus_relative"], key=lambda s: s.rank):
                        rows = [(per[s.rank], name) for name, per in periods["kernel_periods"].items() if s.rank in per]
                        if rows:
                            rec, name = max(rows, key=lambda x: x[0]["excess"])
                            print(f"step {step}:   rank {s.rank}: {name} is {rec['excess']:.2f}x slower every {rec['period']} samples, "
                                  f"last {rec['samples_ago']} samples ago (of {rec['window']}; the beat explains {rec['strength']:.2f} "
                                  f"of the row's variance)")
                episodes = report.episode_scores()  # {} unless NVRX_EPISODE_DETECTION=1 asks for episode scores
                if episodes:
                    print(f"step {step}: GPUs relative episode perf: { {r: round(s, 3) for r, s in episodes['gpu_scores'].items()} }")
                    episode_found = report.identify_episode_stragglers(gpu_rel_threshold=args.threshold)
                    if episode_found["straggler_gpus_relative"]:
                        print(f"step {step}: episode straggler_gpus_relative: "
                              f"{sorted((s.rank, s.node) for s in episode_found['straggler_gpus_relative'])}")
                    for s in sorted(episode_found["straggler_gpus_relative"], key=lambda s: s.rank):
                        rows = [(per[s.rank], name) for name, per in episodes["kernel_episodes"].items() if s.rank in per]
                        if rows:
                            rec, name = max(rows, key=lambda x: x[0]["excess"])
                            print(f"step {step}:   rank {s.rank}: {name} was {rec['excess']:.2f}x slower for {rec['length']} samples "
                                  f"that ended {rec['samples_ago']} samples ago (of {rec['window']}; the stretch explains "
                                  f"{rec['strength']:.2f} of the row's variance{', and has not ended' if rec['open_ended'] else ''})")
                print(f"step {step}: {straggler.Detector.gpu_telemetry_line()}", flush=True)
    if slow_ctx is not None:
        slow_ctx.__exit__(None, None, None)
    torch.cuda.synchronize()
    if rank == 0:
        print(f"time per step [ms]: {(time.monotonic() - t_start) / args.steps * 1e3:.3f}")
    straggler.Detector.shutdown()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def persist(reports: int = 20, ranks: int = 8, sections: int = 4, samples: int = 33) -> None:
    """One slow window against a rank that stays slow: what a report flags, and what the score history does."""
    import numpy as np

    from nvrx_straggler.folded import FoldedJob

    torch.cuda.set_device(0)
    job = FoldedJob(total_ranks=ranks, sections=sections, ring_cap=64, scores_to_compute=("relative_perf_scores",),
                    score_history=8, persistence_min_reports=3)

    def named(found):
        return sorted({s.rank for v in found.values() for group in (v.values() if isinstance(v, dict) else [v]) for s in group})

    try:
        for i in range(reports):
            x = 1000.0 * (1.0 + 0.01 * np.random.default_rng([17, i]).standard_normal((ranks, sections, samples)))
            if i == 6:
                x[2] *= 1.6
            if i >= 10:
                x[5] *= 1.45
            for lr, r in enumerate(job.logical_ranks()):
                job.load(lr, x[r].astype(np.float32))
            report = job.report()
            history = report.score_history()
            rec = history["section_relative"][job.section_names[0]]
            print(f"report {i:2d}: flagged {named(report.identify_stragglers())}, for 3 reports in a row "
                  f"{named(report.identify_persistent_stragglers())}; rank 5 on {job.section_names[0]}: latest "
                  f"{rec[5]['latest']:.2f}, median of the last {history['depth']} {rec[5]['median']:.2f}, streak {rec[5]['streak']}, "
                  f"below in {rec[5]['below']} of {rec[5]['present']}")
    finally:
        job.close()


def trend(reports: int = 48, ranks: int = 8, sections: int = 4, samples: int = 33) -> None:
    """A rank that loses a percent per report against one bad window: what the score trends say, and when."""
    import numpy as np

    from nvrx_straggler.folded import FoldedJob

    torch.cuda.set_device(0)
    job = FoldedJob(total_ranks=ranks, sections=sections, ring_cap=64, scores_to_compute=("relative_perf_scores",),
                    score_history=16, persistence_min_reports=3, score_trends=True)

    def named(found):
        return sorted({s.rank for v in found.values() for group in (v.values() if isinstance(v, dict) else [v]) for s in group})

    first = {}
    try:
        for i in range(reports):
            x = 1000.0 * (1.0 + 0.01 * np.random.default_rng([23, i]).standard_normal((ranks, sections, samples)))
            x[5] *= 1.0 + 0.012 * max(0, i - 8)
            if i == 14:
                x[2] *= 1.4
            for lr, r in enumerate(job.logical_ranks()):
                job.load(lr, x[r].astype(np.float32))
            report = job.report()
            rules = {"declining": named(report.identify_declining_stragglers()), "flagged": named(report.identify_stragglers()),
                     "persistent": named(report.identify_persistent_stragglers())}
            for rule, ranks_named in rules.items():
                if 5 in ranks_named:
                    first.setdefault(rule, i)
            rec = report.score_trends()["section_relative"][job.section_names[0]][5]
            print(f"report {i:2d}: declining {rules['declining']}, flagged {rules['flagged']}, for 3 reports in a row "
                  f"{rules['persistent']}; rank 5 on {job.section_names[0]}: slope {rec['slope']:+.4f} per report, level "
                  f"{rec['level']:.3f}, tau {rec['tau']:+.2f}, reports_left {rec['reports_left']}")
        print("rank 5 first named: " + ", ".join(f"{rule} at report {first.get(rule)}" for rule in ("declining", "flagged", "persistent")))
    finally:
        job.close()


def slack(ranks: int = 8, calls: int = 200, late_rank: int = 5, late_us: float = 300.0) -> None:
    """A rank whose host is slow: every score reads 1, the slack scores name it and say what the job loses."""
    import numpy as np

    from nvrx_straggler.folded import FoldedJob

    torch.cuda.set_device(0)
    gemm, allreduce = "gemm_kernel<bf16>", "ncclDevKernel_AllReduce_Sum_bf16_RING_LL(ncclDevKernelArgsStorage<4096ul>)"
    job = FoldedJob(total_ranks=ranks, section_names=["step"], ring_cap=256, scores_to_compute=("relative_perf_scores",),
                    collective_slack=True, kernel_names=[gemm, allreduce])
    rng = np.random.default_rng(17)
    transfer = 200.0 * (1.0 + 0.02 * rng.standard_normal(calls))
    arrival = rng.exponential(20.0, (ranks, calls))
    arrival[late_rank] += late_us
    last = arrival.max(0)
    in_collective = transfer[None, :] + last[None, :] - arrival  # a rank waits for the last one, then the transfer runs
    step = 1000.0 + transfer + last                              # the step ends with the collective: the same everywhere

    def named(found):
        return sorted({s.rank for v in found.values() for group in (v.values() if isinstance(v, dict) else [v]) for s in group})

    try:
        for lr, r in enumerate(job.logical_ranks()):
            job.load(lr, step[None, :].astype(np.float32))
            job.load_kernels(lr, np.stack([np.full(calls, 1000.0), in_collective[r]]).astype(np.float32))
        report = job.report()
        s = report.slack_scores()
        print(f"identify_stragglers(): {named(report.identify_stragglers())}; lowest relative GPU score "
              f"{min(report.gpu_relative_perf_scores.values()):.3f}")
        print(f"identify_slack_stragglers(): {named(report.identify_slack_stragglers())}; the typical rank waits "
              f"{s['typical_waited_us']:.0f} us per window, {100 * s['typical_share']:.1f} % of its traced GPU time")
        for r, rec in sorted(s["ranks"].items()):
            print(f"  rank {r}: {rec['calls']} calls, in collectives {rec['collective_us']:.0f} us, waited {rec['waited_us']:.0f} us "
                  f"(share {rec['share']:.3f}), the others wait {rec['lead_us']:.0f} us for it")
    finally:
        job.close()


def slack_peer(calls: int = 200, late_rank: int = 5, late_us: float = 300.0) -> None:
    """A pipeline job of two stages (2 + 6 ranks) whose waits in collectives differ per stage, and a rank of the second stage
    whose host is slow: whom the job-wide slack rule names, and whom the rule per peer group does."""
    import numpy as np

    from nvrx_straggler.folded import FoldedJob

    torch.cuda.set_device(0)
    stage = np.array([0, 0, 1, 1, 1, 1, 1, 1])
    ranks = stage.size
    gemm, allreduce = "gemm_kernel<bf16>", "ncclDevKernel_AllReduce_Sum_bf16_RING_LL(ncclDevKernelArgsStorage<4096ul>)"
    sendrecv = "ncclDevKernel_SendRecv(ncclDevKernelArgsStorage<4096ul>)"
    rng = np.random.default_rng(17)
    transfer = 200.0 * (1.0 + 0.02 * rng.standard_normal(calls))
    arrival = rng.exponential(20.0, (ranks, calls))
    noise = rng.standard_normal((ranks, calls))
    arrival[late_rank] += late_us
    # the all-reduce is stage-local: a rank waits for the last one OF ITS STAGE; the send / receive bubble differs per stage
    last = np.stack([arrival[stage == stage[r]].max(0) for r in range(ranks)])
    in_allreduce = transfer[None, :] + last - arrival
    bubble = np.array([60.0, 420.0])[stage][:, None] * (1.0 + 0.02 * noise)
    step = 1000.0 + in_allreduce + bubble

    def named(found):
        return sorted({s.rank for v in found.values() for group in (v.values() if isinstance(v, dict) else [v]) for s in group})

    for on in (False, True):
        job = FoldedJob(total_ranks=ranks, section_names=["step"], ring_cap=256, scores_to_compute=("relative_perf_scores",),
                        collective_slack=True, kernel_names=[gemm, allreduce, sendrecv], peer_groups=stage.tolist(),
                        slack_peer_groups=on)
        try:
            for lr, r in enumerate(job.logical_ranks()):
                job.load(lr, step[r][None, :].astype(np.float32))
                job.load_kernels(lr, np.stack([np.full(calls, 1000.0), in_allreduce[r], bubble[r]]).astype(np.float32))
            report = job.report()
            s = report.slack_scores()
            print(f"identify_slack_stragglers() with slack_peer_groups={on}: {named(report.identify_slack_stragglers())}")
            if on:
                for label, g in s["per_group"].items():
                    print(f"  stage {label} (ranks {s['groups'][label]}): the typical rank waits {g['typical_waited_us']:.0f} us per "
                          f"window, {100 * g['typical_share']:.1f} % of its traced GPU time")
            else:
                print(f"  the typical rank of the job waits {s['typical_waited_us']:.0f} us per window, "
                      f"{100 * s['typical_share']:.1f} % of its traced GPU time")
            for r, rec in sorted(s["ranks"].items()):
                print(f"  rank {r}: in collectives {rec['collective_us']:.0f} us, waited {rec['waited_us']:.0f} us "
                      f"(share {rec['share']:.3f}), the others wait {rec['lead_us']:.0f} us for it")
        finally:
            job.close()


def tail_peer_samples(ranks: int = 8, sections: int = 2, samples: int = 2000, slow_rank: int = 6):
    """The ``--tail-peer`` job: ``[ranks, sections, samples]`` f64 microseconds (NumPy only).  The two stages of ``--peer``
    (1000 us and 1500 us, 1 % noise); ``slow_rank`` is 1.5 x slower on every 10th of its samples only."""
    import numpy as np

    x = np.repeat(np.array([1000.0] * (ranks // 2) + [1500.0] * (ranks - ranks // 2)), sections * samples).reshape(ranks, sections, samples)
    x *= 1.0 + 0.01 * np.random.default_rng(31).standard_normal(x.shape)
    x[slow_rank, :, 9::10] *= 1.5
    return x


def period_peer_samples(ranks: int = 8, sections: int = 2, samples: int = 2000, alone: int = 2, every: int = 50):
    """The ``--period-peer`` job: ``[ranks, sections, samples]`` f64 microseconds (NumPy only).  The two stages of ``--peer``;
    a stage-local checkpoint shard makes every rank of stage 1 stall 1.5 x on every ``every``-th sample, and rank ``alone`` of
    stage 0 stalls the same way on its own."""
    import numpy as np

    x = np.repeat(np.array([1000.0] * (ranks // 2) + [1500.0] * (ranks - ranks // 2)), sections * samples).reshape(ranks, sections, samples)
    x *= 1.0 + 0.01 * np.random.default_rng(37).standard_normal(x.shape)
    x[ranks // 2:, :, every - 1::every] *= 1.5
    x[alone, :, every - 1::every] *= 1.5
    return x


def named_ranks(found) -> list:
    """The ranks an ``identify_*_stragglers()`` result names, in any of its mappings."""
    return sorted({s.rank for v in found.values() for group in (v.values() if isinstance(v, dict) else [v]) for s in group})


def row_peer(family: str) -> None:
    """A pipeline job of two stages of different length under a row family's job-wide rule and its rule per peer group
    (``row_peer_groups``): ``tail`` -- rank 6 is slow on a tenth of its samples only; ``period`` -- stage 1 stalls together on a
    beat, rank 2 of stage 0 stalls alone."""
    import numpy as np

    from nvrx_straggler.folded import FoldedJob

    torch.cuda.set_device(0)
    x = tail_peer_samples() if family == "tail" else period_peer_samples()
    ranks, sections, samples = x.shape
    option = {"tail_quantile": 0.95} if family == "tail" else {"period_detection": True}
    for on in (False, True):
        job = FoldedJob(total_ranks=ranks, sections=sections, ring_cap=2048, scores_to_compute=("relative_perf_scores",),
                        peer_groups=f"block:{ranks // 2}", row_peer_groups=on, **option)
        try:
            for lr, r in enumerate(job.logical_ranks()):
                job.load(lr, x[r].astype(np.float32))
            report = job.report()
            scores = getattr(report, family + "_scores")()
            found = getattr(report, f"identify_{family}_stragglers")()
            name = job.section_names[0]
            print(f"identify_{family}_stragglers() with row_peer_groups={on}: {named_ranks(found)}")
            if family == "tail":
                print(f"identify_peer_stragglers(): {named_ranks(report.identify_peer_stragglers())}")
            for r in sorted(scores["section_relative"][name]):
                against = f"its peers (group {scores['group_of'][r]})" if on else "the job"
                print(f"  rank {r}: {name} against {against} {scores['section_relative'][name][r]:.3f}")
            if on:
                for label, ref in scores["section_reference"][name].items():
                    print(f"  group {label} (ranks {scores['groups'][label]}): reference {ref['value']:.3f}, held by rank {ref['rank']}")
        finally:
            job.close()


def peer(ranks: int = 8, sections: int = 4, samples: int = 33, slow_rank: int = 6) -> None:
    """Two pipeline stages of different length: whom the job-wide rule names, and whom the peer-group scores do."""
    import numpy as np

    from nvrx_straggler.folded import FoldedJob

    torch.cuda.set_device(0)
    job = FoldedJob(total_ranks=ranks, sections=sections, ring_cap=64, scores_to_compute=("relative_perf_scores",),
                    peer_groups=f"block:{ranks // 2}")
    x = np.repeat(np.array([1000.0] * (ranks // 2) + [1500.0] * (ranks - ranks // 2)), sections * samples).reshape(ranks, sections, samples)
    x *= 1.0 + 0.01 * np.random.default_rng(29).standard_normal(x.shape)
    x[slow_rank] *= 1.4

    def named(found):
        return sorted({s.rank for v in found.values() for group in (v.values() if isinstance(v, dict) else [v]) for s in group})

    try:
        for lr, r in enumerate(job.logical_ranks()):
            job.load(lr, x[r].astype(np.float32))
        report = job.report()
        t = report.peer_scores()
        name = job.section_names[0]
        print(f"identify_stragglers(): {named(report.identify_stragglers())}")
        print(f"identify_peer_stragglers(): {named(report.identify_peer_stragglers())}; groups {t['groups']}")
        for r in sorted(t["group_of"]):
            print(f"  rank {r} (group {t['group_of'][r]}): {name} against the job "
                  f"{report.section_relative_perf_scores[name][r]:.3f}, against its peers {t['section_relative'][name][r]:.3f}")
    finally:
        job.close()


def peer_persist_windows(reports: int = 16, ranks: int = 8, sections: int = 4, samples: int = 33):
    """The ``--peer-persist`` job, report by report: ``[ranks, sections, samples]`` f64 microseconds (NumPy only)."""
    import numpy as np

    for i in range(reports):
        x = np.repeat(np.array([1000.0] * (ranks // 2) + [1500.0] * (ranks - ranks // 2)), sections * samples)
        x = x.reshape(ranks, sections, samples) * (1.0 + 0.01 * np.random.default_rng([37, i]).standard_normal((ranks, sections, samples)))
        if i == 6:
            x[1] *= 1.6
        if i >= 10:
            x[6] *= 1.4
        yield x


def peer_persist_verdicts(report):
    """``(per-report peer flagging, the job-wide history, the peer history)``: the ranks each rule names, sorted."""
    def named(found):
        return sorted({s.rank for v in found.values() for group in (v.values() if isinstance(v, dict) else [v]) for s in group})

    return (named(report.identify_peer_stragglers()), named(report.identify_persistent_stragglers()),
            named(report.identify_persistent_peer_stragglers()))


def peer_persist(ranks: int = 8) -> None:
    """A pipeline job over 16 reports: one bad window and a rank that stays slower than its peers, under three rules."""
    import numpy as np

    from nvrx_straggler.folded import FoldedJob

    torch.cuda.set_device(0)
    job = FoldedJob(total_ranks=ranks, sections=4, ring_cap=64, scores_to_compute=("relative_perf_scores",),
                    peer_groups=f"block:{ranks // 2}", score_history=8, persistence_min_reports=3, peer_history=8,
                    peer_persistence_min_reports=3)
    try:
        for i, x in enumerate(peer_persist_windows(ranks=ranks)):
            for lr, r in enumerate(job.logical_ranks()):
                job.load(lr, x[r].astype(np.float32))
            report = job.report()
            per_report, job_wide, peers = peer_persist_verdicts(report)
            rec = report.peer_history()["section_relative"][job.section_names[0]][6]
            print(f"report {i:2d}: identify_peer_stragglers() {per_report}, identify_persistent_stragglers() {job_wide}, "
                  f"identify_persistent_peer_stragglers() {peers}; rank 6 against its peers on {job.section_names[0]}: latest "
                  f"{rec['latest']:.2f}, streak {rec['streak']}, below in {rec['below']} of {rec['present']}")
    finally:
        job.close()


def work(ranks: int = 8, sections: int = 4, shared: int = 100, own: int = 10, calls=(1600, 2400), slow_rank: int = 6) -> None:
    """Two pipeline stages nobody described: whom the job-wide rule names, whom ``peer_groups="auto"`` names, and the groups."""
    import numpy as np

    from nvrx_straggler.folded import FoldedJob

    torch.cuda.set_device(0)
    names = [f"kernel_{k:03d}" for k in range(shared + 2 * own)]
    job = FoldedJob(total_ranks=ranks, sections=sections, ring_cap=4096, scores_to_compute=("relative_perf_scores",),
                    kernel_names=names, peer_groups="auto")
    rng = np.random.default_rng(31)
    base = rng.uniform(20.0, 400.0, len(names))

    def named(found):
        return sorted({s.rank for v in found.values() for group in (v.values() if isinstance(v, dict) else [v]) for s in group})

    try:
        for lr, r in enumerate(job.logical_ranks()):
            stage = r // (ranks // 2)
            slow = 1.4 if r == slow_rank else 1.0
            sec = np.full((sections, 33), (1000.0, 1500.0)[stage] * slow) * (1.0 + 0.01 * rng.standard_normal((sections, 33)))
            job.load(lr, sec.astype(np.float32))
            mine = list(range(shared)) + list(range(shared + own * stage, shared + own * (stage + 1)))
            for k in mine:  # (a key of the other stage gets no sample: this rank does not have it)
                n = calls[stage] if k < shared else 200
                job.rings.push_many(job._no_kernel_rows[names[k]], (base[k] * slow * (1.0 + 0.01 * rng.standard_normal(n))).astype(np.float32), lr=lr)
        report = job.report()
        w, t = report.work_groups(), report.peer_scores()
        print(f"identify_stragglers(): {named(report.identify_stragglers())}")
        print(f"identify_peer_stragglers() with peer_groups='auto': {named(report.identify_peer_stragglers())}")
        print(f"inferred groups: {w['groups']}; rule {w['params']}")
        for r in sorted(w["ranks"]):
            d = w["ranks"][r]
            print(f"  rank {r} (group {w['group_of'][r]} of {d['size']}): {d['kernels']} kernels, {d['sections']} sections; nearest rank "
                  f"{d['nearest']} differs in {d['nearest_unlike']} of {d['nearest_columns']} columns; relative GPU score against the job "
                  f"{report.gpu_relative_perf_scores[r]:.3f}, against its peers {t['gpu_relative'][r]:.3f}")
    finally:
        job.close()


def pace(ranks: int = 8, kernels: int = 120, calls: int = 200, slow_rank: int = 5, slowdown: float = 1.04) -> None:
    """A rank that is a little slower in everything: whom the threshold rules name, and whom the pace scores do."""
    import numpy as np

    from nvrx_straggler.folded import FoldedJob

    torch.cuda.set_device(0)
    names = [f"kernel_{k:03d}" for k in range(kernels)]
    job = FoldedJob(total_ranks=ranks, section_names=["step"], ring_cap=256, scores_to_compute=("relative_perf_scores",),
                    kernel_names=names, robust_scores=True, pace_scores=True)
    rng = np.random.default_rng(2026)
    med = rng.lognormal(np.log(100.0), 0.5, kernels)[None, :] * (1.0 + 0.01 * rng.standard_normal((ranks, kernels)))
    med[slow_rank] *= slowdown
    med = med.astype(np.float32)

    def named(found):
        return sorted({s.rank for v in found.values() for group in (v.values() if isinstance(v, dict) else [v]) for s in group})

    try:
        for lr, r in enumerate(job.logical_ranks()):
            job.load(lr, np.full((1, calls), med[r].sum(), dtype=np.float32))
            job.load_kernels(lr, np.repeat(med[r][:, None], calls, axis=1))
        report = job.report()
        t = report.pace_scores()
        robust = report.robust_scores()
        print(f"identify_stragglers(): {named(report.identify_stragglers())}")
        print(f"identify_robust_stragglers(): {named(report.identify_robust_stragglers())}")
        print(f"identify_pace_stragglers(): {named(report.identify_pace_stragglers())}; rule {t['params']}")
        for r in sorted(t["ranks"]):
            gpu = t["ranks"][r]["gpu"]
            print(f"  rank {r}: relative GPU score {report.gpu_relative_perf_scores[r]:.3f}, robust z {robust['gpu_z'][r]:+.2f}, "
                  f"pace {gpu['pace']:.3f} (spread {gpu['spread']:.3f}), slower / faster than the job's median in "
                  f"{gpu['slower']} / {gpu['faster']} of {gpu['columns']} kernels, {gpu['excess_us']:+.0f} us above its pace")
    finally:
        job.close()


def pace_peer(ranks: int = 8, kernels: int = 120, calls: int = 200, stage: int = 4, slow_rank: int = 6,
              slowdown: float = 1.04, seed: int = 2026) -> None:
    """A degraded GPU in a pipeline job: whom the job-wide pace rule names, and whom the rule per peer group does."""
    import numpy as np

    from nvrx_straggler.folded import FoldedJob

    torch.cuda.set_device(0)
    names = [f"kernel_{k:03d}" for k in range(kernels)]
    rng = np.random.default_rng(seed)
    med = rng.lognormal(np.log(100.0), 0.5, kernels)[None, :] * (1.0 + 0.01 * rng.standard_normal((ranks, kernels)))
    med[(np.arange(ranks) // stage) % 2 == 1] *= 1.5  # the odd stages are 1.5 x slower
    med[slow_rank] *= slowdown
    med = med.astype(np.float32)

    def named(found):
        return sorted({s.rank for v in found.values() for group in (v.values() if isinstance(v, dict) else [v]) for s in group})

    for title, grouped in (("job-wide", False), ("per-peer-group", True)):
        job = FoldedJob(total_ranks=ranks, section_names=["step"], ring_cap=256, scores_to_compute=("relative_perf_scores",),
                        kernel_names=names, pace_scores=True, peer_groups=f"block:{stage}", pace_peer_groups=grouped)
        try:
            for lr, r in enumerate(job.logical_ranks()):
                job.load(lr, np.full((1, calls), med[r].sum(), dtype=np.float32))
                job.load_kernels(lr, np.repeat(med[r][:, None], calls, axis=1))
            report = job.report()
            t = report.pace_scores()
            print(f"identify_pace_stragglers() {title}: {named(report.identify_pace_stragglers())}; rule {t['params']}")
            for r in sorted(t["ranks"]):
                gpu = t["ranks"][r]["gpu"]
                against = f"group {t['group_of'][r]}'s" if grouped else "the job's"
                print(f"  rank {r}: pace {gpu['pace']:.3f} (spread {gpu['spread']:.3f}), slower / faster than {against} median in "
                      f"{gpu['slower']} / {gpu['faster']} of {gpu['columns']} kernels, {gpu['excess_us']:+.0f} us above its pace")
        finally:
            job.close()


def node(ranks: int = 32, per_node: int = 8, kernels: int = 120, calls: int = 200, slow_node: int = 2, slow_rank: int = 5,
         slowdown: float = 1.04, seed: int = 2026) -> None:
    """A slow host and a slow GPU in one job: whom the pace rule names, and what the node rule makes of them."""
    import numpy as np

    from nvrx_straggler.folded import FoldedJob

    torch.cuda.set_device(0)
    names = [f"kernel_{k:03d}" for k in range(kernels)]
    rng = np.random.default_rng(seed)
    med = rng.lognormal(np.log(100.0), 0.5, kernels)[None, :] * (1.0 + 0.01 * rng.standard_normal((ranks, kernels)))
    med[slow_node * per_node : (slow_node + 1) * per_node] *= slowdown  # the whole node
    med[slow_rank] *= slowdown                                          # one card elsewhere
    med = med.astype(np.float32)
    job = FoldedJob(total_ranks=ranks, section_names=["step"], ring_cap=256, scores_to_compute=("relative_perf_scores",),
                    kernel_names=names, pace_scores=True, node_scores=True, node_groups=f"block:{per_node}")
    try:
        for lr, r in enumerate(job.logical_ranks()):
            job.load(lr, np.full((1, calls), med[r].sum(), dtype=np.float32))
            job.load_kernels(lr, np.repeat(med[r][:, None], calls, axis=1))
        report = job.report()
        t = report.node_scores()
        found = report.identify_node_stragglers()
        print(f"identify_pace_stragglers(): {sorted(s.rank for s in report.identify_pace_stragglers()['straggler_gpus_relative'])}")
        print(f"identify_node_stragglers() nodes: {sorted(found['straggler_nodes'])}; rule {t['params']}")
        print(f"identify_node_stragglers() ranks off pace alone: {sorted(s.rank for s in found['ranks_off_pace_alone'])}")
        for label in sorted(t["node_scores"]):
            d = t["node_scores"][label]
            gpu = d["gpu"]
            print(f"  node {label} (ranks {t['nodes'][label][0]}-{t['nodes'][label][-1]}): pace {gpu['pace']:.4f} (spread "
                  f"{gpu['spread']:.4f}), slower / faster than the nodes' median in {gpu['slower']} / {gpu['faster']} of "
                  f"{gpu['columns']} kernels, {d['members_off_pace']} of {d['members_rated']} ranks off pace")
        for r in sorted(s.rank for s in found["ranks_off_pace_alone"]):
            gpu = t["ranks"][r]["gpu"]
            print(f"  rank {r} (node {t['node_of'][r]}): pace {gpu['pace']:.3f}, slower in {gpu['slower']} of {gpu['columns']} "
                  f"kernels, {gpu['excess_us']:+.0f} us above the nodes' pace")
    finally:
        job.close()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-processes", type=int, default=1)
    ap.add_argument("--share-gpu", action="store_true", help="all ranks on GPU 0 over gloo (a box with one GPU)")
    ap.add_argument("--steps", type=int, default=900)
    ap.add_argument("--batch-size", type=int, default=4096)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--report-interval", type=int, default=300)
    ap.add_argument("--threshold", type=float, default=0.75)
    ap.add_argument("--slow-rank", type=int, default=-1)
    ap.add_argument("--slow-from", type=int, default=300)
    ap.add_argument("--slow-by", choices=["clock", "simulated", "intermittent", "onset", "stretch"], default="clock")
    ap.add_argument("--slow-every", type=int, default=5,
                    help="--slow-by intermittent: the slow rank's stand-in kernel is 1.5x longer on every N-th step only (with one "
                         "step in ten slow, a 0.9 quantile would sit on the last FAST sample)")
    ap.add_argument("--simulated-cycles", type=float, default=3e6, help="--slow-by simulated: spin cycles of the stand-in kernel")
    ap.add_argument("--persist", action="store_true",
                    help="no training: play the score-history scenario (one slow window against a rank that stays slow) and exit")
    ap.add_argument("--trend", action="store_true",
                    help="no training: play the score-trend scenario (a rank that loses a percent per report against one bad "
                         "window) and exit")
    ap.add_argument("--slack", action="store_true",
                    help="no training: play the slack-score scenario (a rank whose host is slow arrives late at every "
                         "collective) and exit")
    ap.add_argument("--slack-peer", action="store_true",
                    help="no training: play the slack-score scenario of a pipeline job (stages of 2 and 6 ranks whose waits in "
                         "collectives differ, rank 5 arriving late) with the job-wide rule and the rule per peer group, and exit")
    ap.add_argument("--tail-peer", action="store_true",
                    help="no training: play the tail-score scenario of a pipeline job (the two stages of --peer, rank 6 1.5 x "
                         "slower on a tenth of its samples) with the job-wide rule and the rule per peer group, and exit")
    ap.add_argument("--period-peer", action="store_true",
                    help="no training: play the period-score scenario of a pipeline job (stage 1 stalls together on every 50th "
                         "sample, rank 2 of stage 0 stalls alone) with the job-wide rule and the rule per peer group, and exit")
    ap.add_argument("--peer", action="store_true",
                    help="no training: play the peer-group scenario (two pipeline stages of different length, one rank slow "
                         "within its stage) and exit")
    ap.add_argument("--peer-persist", action="store_true",
                    help="no training: play the peer-history scenario (the two stages of --peer over 16 reports: one bad "
                         "window of rank 1, rank 6 slower than its stage from report 10 on) under three rules, and exit")
    ap.add_argument("--pace", action="store_true",
                    help="no training: play the pace-score scenario (a rank 4 %% slower in every one of its 120 kernels) and "
                         "exit")
    ap.add_argument("--pace-peer", action="store_true",
                    help="no training: play the pace-score scenario of a pipeline job (two stages, the second 1.5 x slower, rank 6 "
                         "4 %% slower than its stage in every kernel) with the job-wide rule and the rule per peer group, and exit")
    ap.add_argument("--node", action="store_true",
                    help="no training: play the node-score scenario (32 ranks on 4 nodes, every rank of node 2 and rank 5 of node "
                         "0 4 %% slower in every kernel) with the pace rule and the node rule, and exit")
    ap.add_argument("--work", action="store_true",
                    help="no training: play the work-group scenario (the two pipeline stages of --peer with nobody describing "
                         "the layout: the groups are inferred from the kernels each rank runs and how often) and exit")
    args = ap.parse_args()
    if args.work:
        work()
        return
    if args.tail_peer or args.period_peer:
        row_peer("tail" if args.tail_peer else "period")
        return
    if args.node:
        node()
        return
    if args.pace_peer:
        pace_peer()
        return
    if args.pace:
        pace()
        return
    if args.slack_peer:
        slack_peer()
        return
    if args.slack:
        slack()
        return
    if args.peer_persist:
        peer_persist()
        return
    if args.peer:
        peer()
        return
    if args.persist:
        persist()
        return
    if args.trend:
        trend()
        return
    if "RANK" in os.environ or args.num_processes == 1:
        train(args)
        return
    with socket.socket() as s:   # one process per rank, the environment torchrun would give them, rendezvous on 127.0.0.1
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = [subprocess.Popen([sys.executable] + sys.argv,
                              env=dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.num_processes),
                                       MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0"))
             for r in range(args.num_processes)]
    rc = 0
    for p in procs:
        rc = p.wait() or rc
    sys.exit(rc)


if __name__ == "__main__":
    main()
