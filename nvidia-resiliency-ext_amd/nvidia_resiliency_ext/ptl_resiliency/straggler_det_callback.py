"""``StragglerDetectionCallback``: PyTorch-Lightning hook-up of the MI355X straggler detector.

Constructor arguments, hooks (``setup / teardown / on_train_batch_end``), log texts and the
stop-on-straggler behaviour follow the reference callback (ptl_resiliency/straggler_det_callback.py:
37-265).  Differences: Lightning is optional -- if neither ``lightning`` nor ``pytorch_lightning`` is
installed the callback derives from ``object`` and still works with any trainer exposing the same
hooks -- and the rank-0 "stragglers found" broadcast travels on the process group's own device.
"""
from __future__ import annotations

import importlib.util
import logging
import sys
import time
from typing import Optional

import torch

import nvrx_straggler as straggler
from nvrx_straggler import dist_utils


def _callback_base():
    for mod in ("lightning.pytorch.callbacks", "pytorch_lightning.callbacks"):
        try:
            if importlib.util.find_spec(mod.split(".")[0]) is not None:
                return importlib.import_module(mod).Callback
        except (ImportError, ValueError):
            continue
    return object


Callback = _callback_base()


class StragglerDetectionCallback(Callback):
    def __init__(
        self,
        report_time_interval: float,
        calc_relative_gpu_perf: bool,
        calc_individual_gpu_perf: bool,
        num_gpu_perf_scores_to_print: int,
        gpu_relative_perf_threshold: float,
        gpu_individual_perf_threshold: float,
        stop_if_detected: bool,
        enable_ptl_logging: bool,
        profiling_interval: int = 1,
        logger_name: Optional[str] = "nemo_logger.StragglerDetectionCallback",
        min_consecutive_reports: int = 1,
        warn_if_declining: bool = False,
        warn_if_waited_for: bool = False,
        peer_groups=None,
        warn_if_off_pace: bool = False,
        pace_peer_groups: bool = False,
        warn_if_node_off_pace: bool = False,
        node_groups=None,
        min_consecutive_peer_reports: int = 1,
        slack_peer_groups: bool = False,
    ):
        """
        Args:
            report_time_interval: seconds between straggler checks.
            calc_relative_gpu_perf / calc_individual_gpu_perf: which score families to compute.
            num_gpu_perf_scores_to_print: how many best and worst ranks to print each report
                (0: print only when stragglers are found).
            gpu_relative_perf_threshold / gpu_individual_perf_threshold: flagging thresholds.
            stop_if_detected: stop training (after a final checkpoint) when stragglers are found.
            enable_ptl_logging: log min/median/max GPU scores through ``pl_module.log_dict``.
            profiling_interval: forwarded to ``Detector.initialize``.
            logger_name: name of the ``logging`` logger to use.
            min_consecutive_reports: 1 (the default, the reference's behaviour): a GPU is reported, and with
                ``stop_if_detected`` the job is stopped, the first time a report flags it.  M > 1: only once its score has
                been below the threshold in M reports in a row (``Report.identify_persistent_stragglers``; the detector
                then keeps a score history of ``max(8, M)`` reports): one slow window -- a neighbour's checkpoint, a
                page-cache flush -- no longer ends a healthy job.  Every report's scores are printed and logged as before.
            warn_if_declining: False (the default): nothing changes.  True: the detector keeps a score history of at least 8
                reports with score trends (``Detector.initialize(score_trends=True)``), and every report that finds a GPU
                whose score is falling towards its threshold (``Report.identify_declining_stragglers``) logs one warning
                that names the ranks and the reports left until they cross it.  A warning only: it never stops the job.
            warn_if_waited_for: False (the default): nothing changes.  True: the detector also computes slack scores
                (``Detector.initialize(collective_slack=True)``; per-kernel timing only), and every report in which the job
                waits for some rank in its collectives (``Report.identify_slack_stragglers``: a slow HOST, which no other
                score sees) logs one warning that names the ranks and the microseconds the others wait for each per report
                window.  A warning only: it never stops the job.
            peer_groups: None (the default): nothing changes.  Otherwise which ranks do the same work, as
                ``Detector.initialize(peer_groups=...)`` takes it: labels, one per rank, or ``"block:N"`` / ``"mod:N"``.  ``"auto"``: nobody
                describes the layout; every report infers the groups from its table (``Report.work_groups()``).  The
                RELATIVE family's warning, and with ``stop_if_detected`` the halt, then come from
                ``Report.identify_peer_stragglers`` -- each rank against the fastest rank of its own group -- so that the
                healthy ranks of a slower pipeline stage do not stop the job.  Ranks without a peer are unrated; they are
                logged once.  The individual family is untouched.
            warn_if_off_pace: False (the default): nothing changes.  True: the detector also computes pace scores
                (``Detector.initialize(pace_scores=True)``), and every report that finds a GPU a little slower than the job's
                median in nearly all of its kernels (``Report.identify_pace_stragglers``: a degraded card, which no threshold
                on one score sees) logs one warning that names the ranks with their pace and the microseconds they spent
                above the job's median pace.  A warning only: it never stops the job.
            pace_peer_groups: False (the default): nothing changes.  True (needs ``warn_if_off_pace`` and ``peer_groups``):
                the pace scores rate each rank against the median of its own peer group
                (``Detector.initialize(pace_peer_groups=True)``), so that the healthy ranks of a slower pipeline stage are not
                warned about at every report, and the warning says the ranks are off their peer group's pace.  Still a
                warning only.
            warn_if_node_off_pace: False (the default): nothing changes.  True: the detector also computes node scores
                (``Detector.initialize(node_scores=True)``), and every report that finds a NODE a little slower than the job's
                nodes in nearly all of its kernels, most of its GPUs agreeing (``Report.identify_node_stragglers``: a host
                fault -- fans, PSU, host CPU, power profile), logs one warning that names the nodes with their pace and how
                many of their GPUs are off pace.  A warning only: it never stops the job.
            node_groups: which ranks share a node, for ``warn_if_node_off_pace`` (None: the node names the detector gathers;
                else ``"block:N"``, ``"mod:N"`` or one label per rank, as ``Detector.initialize(node_groups=...)``).
            min_consecutive_peer_reports: 1 (the default): nothing changes.  M > 1 (needs ``peer_groups``): the relative
                family's warning, and with ``stop_if_detected`` the halt, come only once a GPU's PEER score has been below the
                relative threshold in M reports in a row (``Report.identify_persistent_peer_stragglers``; the detector then
                keeps a peer history of ``max(8, M)`` reports, ``Detector.initialize(peer_history=...)``): what
                ``min_consecutive_reports`` does for a job without peer groups.  With ``peer_groups`` use this, not
                ``min_consecutive_reports``: the job-wide history rates every healthy rank of a slower stage low in every
                report and would name them all from the M-th report on.
            slack_peer_groups: False (the default): nothing changes.  True (needs ``warn_if_waited_for`` and ``peer_groups``):
                the slack scores are taken inside each rank's own peer group
                (``Detector.initialize(slack_peer_groups=True)``), so that a pipeline job is not warned about the healthy ranks
                of the stage that waits least at every report, and the warning names the ranks their own peer group waits
                for.  Still a warning only.

        Raises:
            ValueError: ``slack_peer_groups`` without ``warn_if_waited_for`` or without ``peer_groups``, neither score family requested, ``min_consecutive_reports`` outside [1, 64],
                ``warn_if_waited_for``, ``warn_if_off_pace`` or ``peer_groups`` without ``calc_relative_gpu_perf``, or ``peer_groups`` together with
                ``min_consecutive_reports`` > 1 (the score history does not hold peer scores), or ``pace_peer_groups`` without
                ``warn_if_off_pace`` or without ``peer_groups``, or ``warn_if_node_off_pace`` without ``calc_relative_gpu_perf``, or
                ``min_consecutive_peer_reports`` outside [1, 64] or above 1 without ``peer_groups``.
        """
        self.initialized = False
        self.logger = logging.getLogger(logger_name)
        self.report_time_interval = report_time_interval
        self.calc_relative_gpu_perf = calc_relative_gpu_perf
        self.calc_individual_gpu_perf = calc_individual_gpu_perf
        self.num_gpu_perf_scores_to_print = num_gpu_perf_scores_to_print
        self.gpu_relative_perf_threshold = gpu_relative_perf_threshold
        self.gpu_individual_perf_threshold = gpu_individual_perf_threshold
        self.stop_if_detected = stop_if_detected
        self.enable_ptl_logging = enable_ptl_logging
        self.profiling_interval = profiling_interval
        self.scores_to_compute = []
        if calc_relative_gpu_perf:
            self.scores_to_compute.append("relative_perf_scores")
        if calc_individual_gpu_perf:
            self.scores_to_compute.append("individual_perf_scores")
        if not self.scores_to_compute:
            raise ValueError(
                "No straggler performance scores specified. "
                "Check if calc_relative_gpu_perf=True or calc_individual_gpu_perf=True"
            )
        if (isinstance(min_consecutive_reports, bool) or not isinstance(min_consecutive_reports, int)
                or not 1 <= min_consecutive_reports <= 64):
            raise ValueError(f"min_consecutive_reports must be an integer within [1, 64], got {min_consecutive_reports!r}")
        self.min_consecutive_reports = min_consecutive_reports
        self.warn_if_declining = bool(warn_if_declining)
        self.warn_if_waited_for = bool(warn_if_waited_for)
        if self.warn_if_waited_for and not calc_relative_gpu_perf:
            raise ValueError("warn_if_waited_for needs calc_relative_gpu_perf=True: slack scores compare ranks")
        self.warn_if_off_pace = bool(warn_if_off_pace)
        if self.warn_if_off_pace and not calc_relative_gpu_perf:
            raise ValueError("warn_if_off_pace needs calc_relative_gpu_perf=True: pace scores compare ranks")
        self.peer_groups = peer_groups
        if peer_groups is not None:
            if not calc_relative_gpu_perf:
                raise ValueError("peer_groups needs calc_relative_gpu_perf=True: peer-group scores are relative scores")
            if min_consecutive_reports > 1:
                raise ValueError("peer_groups cannot be combined with min_consecutive_reports > 1: the score history does "
                                 "not hold peer-group scores")
        if (isinstance(min_consecutive_peer_reports, bool) or not isinstance(min_consecutive_peer_reports, int)
                or not 1 <= min_consecutive_peer_reports <= 64):
            raise ValueError(f"min_consecutive_peer_reports must be an integer within [1, 64], "
                             f"got {min_consecutive_peer_reports!r}")
        if min_consecutive_peer_reports > 1 and peer_groups is None:
            raise ValueError("min_consecutive_peer_reports > 1 needs peer_groups: it counts reports of the peer-group scores")
        self.min_consecutive_peer_reports = min_consecutive_peer_reports
        self.pace_peer_groups = bool(pace_peer_groups)
        if self.pace_peer_groups:
            if not self.warn_if_off_pace:
                raise ValueError("pace_peer_groups needs warn_if_off_pace=True: it changes what the pace scores compare with")
            if peer_groups is None:
                raise ValueError("pace_peer_groups needs peer_groups: which ranks do the same work")
        self.slack_peer_groups = bool(slack_peer_groups)
        if self.slack_peer_groups:
            if not self.warn_if_waited_for:
                raise ValueError("slack_peer_groups needs warn_if_waited_for=True: it changes what the slack scores compare with")
            if peer_groups is None:
                raise ValueError("slack_peer_groups needs peer_groups: which ranks do the same work")
        self.warn_if_node_off_pace = bool(warn_if_node_off_pace)
        if self.warn_if_node_off_pace and not calc_relative_gpu_perf:
            raise ValueError("warn_if_node_off_pace needs calc_relative_gpu_perf=True: node scores compare nodes")
        self.node_groups = node_groups
        self._unrated_said = False
        self.interval_est_was_reset = False

    # ---- Lightning hooks -----------------------------------------------------------------------
    def setup(self, trainer, pl_module, stage):
        if self.initialized:
            return
        persistence = {}
        if self.min_consecutive_reports > 1:
            m = self.min_consecutive_reports
            persistence = dict(score_history=max(8, m), persistence_min_reports=m,
                               persistence_thresholds=(self.gpu_relative_perf_threshold, 0.75,
                                                       self.gpu_individual_perf_threshold, 0.75))
        if self.warn_if_declining:
            persistence.setdefault("score_history", 8)
            persistence.setdefault("persistence_thresholds", (self.gpu_relative_perf_threshold, 0.75,
                                                              self.gpu_individual_perf_threshold, 0.75))
            persistence["score_trends"] = True
        if self.warn_if_waited_for:
            persistence["collective_slack"] = True
        if self.peer_groups is not None:
            persistence["peer_groups"] = self.peer_groups
        if self.min_consecutive_peer_reports > 1:
            m = self.min_consecutive_peer_reports
            persistence.update(peer_history=max(8, m), peer_persistence_min_reports=m,
                               peer_persistence_thresholds=(self.gpu_relative_perf_threshold, 0.75))
        if self.warn_if_off_pace:
            persistence["pace_scores"] = True
        if self.pace_peer_groups:
            persistence["pace_peer_groups"] = True
        if self.slack_peer_groups:
            persistence["slack_peer_groups"] = True
        if self.warn_if_node_off_pace:
            persistence["node_scores"] = True
            if self.node_groups is not None:
                persistence["node_groups"] = self.node_groups
        straggler.Detector.initialize(
            scores_to_compute=self.scores_to_compute,
            gather_on_rank0=True,
            profiling_interval=self.profiling_interval,
            report_time_interval=self.report_time_interval,
            **persistence,
        )
        step_owner = trainer.strategy
        assert getattr(step_owner, "training_step", None), f"{type(step_owner)} does not have 'training_step' method."
        # every training step becomes a profiled section named "<Strategy class>.training_step"
        straggler.Detector.wrap_callables(callable_ids=[straggler.CallableId(step_owner, "training_step")])
        self.initialized = True

    def teardown(self, trainer, pl_module, stage):
        if self.initialized:
            straggler.Detector.shutdown()
            self.initialized = False

    def on_train_batch_end(self, trainer, pl_module, outputs, batch, batch_idx):
        started = time.monotonic()
        detector = straggler.Detector
        report = detector.generate_report_if_interval_elapsed()
        # gather_on_rank0: rank 0 alone holds the report and decides; the decision reaches the others below
        found = bool(report) and trainer.global_rank == 0 and self._digest(pl_module, report)
        if self.warn_if_declining and bool(report) and trainer.global_rank == 0:
            self._warn_declining(report)  # (a warning only: `found`, and with it the halt, does not depend on it)
        if self.warn_if_waited_for and bool(report) and trainer.global_rank == 0:
            self._warn_waited_for(report)  # (likewise)
        if self.warn_if_off_pace and bool(report) and trainer.global_rank == 0:
            self._warn_off_pace(report)  # (likewise)
        if self.warn_if_node_off_pace and bool(report) and trainer.global_rank == 0:
            self._warn_node_off_pace(report)  # (likewise)
        if not detector.is_interval_elapsed():
            return  # no report was due this iteration
        if self.stop_if_detected and self._decision_of_rank0(found):
            self._halt(trainer)
        self.logger.info(f"Straggler report processing time: {time.monotonic() - started:.3f} sec.")

    # ---- what happens with a report (rank 0) -----------------------------------------------------------
    #: (constructor switch, Report field, identify_stragglers key, heading, logging prefix, warning text)
    _FAMILIES = (
        ("calc_relative_gpu_perf", "gpu_relative_perf_scores", "straggler_gpus_relative", "GPU relative performance",
         "gpu_relative_perf", "Some GPUs have worse relative performance."),
        ("calc_individual_gpu_perf", "gpu_individual_perf_scores", "straggler_gpus_individual", "GPU individual performance",
         "gpu_individual_perf", "Some GPUs performance dropped."),
    )

    def _digest(self, pl_module, report) -> bool:
        """Warn about flagged GPUs, print the best / worst ranks, feed the PTL loggers; True if anything was flagged -- with
        ``min_consecutive_reports`` above 1: flagged in that many reports in a row."""
        m = self.min_consecutive_reports
        if m > 1:
            flagged = report.identify_persistent_stragglers()
        else:
            flagged = report.identify_stragglers(
                gpu_rel_threshold=self.gpu_relative_perf_threshold,
                gpu_indiv_threshold=self.gpu_individual_perf_threshold,
            )
        texts = {}
        if self.peer_groups is not None:
            # the relative family's verdict: each rank against its own group
            flagged = dict(flagged)
            pm = self.min_consecutive_peer_reports
            if pm > 1:
                flagged["straggler_gpus_relative"] = report.identify_persistent_peer_stragglers()["straggler_gpus_relative"]
                texts["straggler_gpus_relative"] = (f"Some GPUs have worse performance than their peer group for {pm} "
                                                    "consecutive reports.")
            else:
                flagged["straggler_gpus_relative"] = report.identify_peer_stragglers(
                    gpu_rel_threshold=self.gpu_relative_perf_threshold)["straggler_gpus_relative"]
                texts["straggler_gpus_relative"] = "Some GPUs have worse performance than their peer group."
            if not self._unrated_said:
                self._unrated_said = True
                unrated = report.peer_scores().get("unrated_ranks", [])
                if unrated:
                    self.logger.info(f"Straggler detection: ranks without a peer in their group are not rated: {unrated}")
        hits = [(texts.get(key, text), flagged[key]) for _, _, key, _, _, text in self._FAMILIES if flagged[key]]
        for text, ranks in hits:
            if m > 1:
                text = f"{text.rstrip('.')} for {m} consecutive reports."
            self.logger.warning(f"STRAGGLER DETECTION WARNING: {text} Affected ranks: {ranks}")
        if hits:
            self._name_the_kernels(report, flagged)
            self._telemetry_of_a_flagged_reporter(ranks for _, ranks in hits)
        enabled = [f for f in self._FAMILIES if getattr(self, f[0])]
        n = self.num_gpu_perf_scores_to_print
        if n > 0:
            for _, field, _, heading, _, _ in enabled:
                self.logger.info(f"\n{heading}:\n{self._ranking(getattr(report, field), report.rank_to_node, n, n)}")
        if self.enable_ptl_logging:
            for _, field, _, _, prefix, _ in enabled:
                self._log_extremes(pl_module, getattr(report, field), prefix)
        return bool(hits)

    def _warn_declining(self, report) -> None:
        """One warning per report that names the GPUs whose score is falling towards its threshold, with the reports left
        until the trend line crosses it (``warn_if_declining``).  Never a reason to halt."""
        declining = report.identify_declining_stragglers()
        trends = report.score_trends()
        parts = []
        for family, key, table in (("relative", "straggler_gpus_relative", "gpu_relative"),
                                   ("individual", "straggler_gpus_individual", "gpu_individual")):
            per_rank = trends.get(table, {})
            for rank in sorted(getattr(s, "rank", s) for s in declining[key]):
                rec = per_rank[rank]
                parts.append(f"rank {rank} {family} GPU score falls {-rec['slope']:.4f} per report "
                             f"(level {rec['level']:.3f}, reports_left={rec['reports_left']})")
        if parts:
            self.logger.warning("STRAGGLER DETECTION WARNING: Some GPUs are getting slower: " + "; ".join(parts))

    def _warn_waited_for(self, report) -> None:
        """One warning per report that names the GPUs the others wait for in collectives, with the time the typical rank
        waits for each per report window (``warn_if_waited_for``).  Never a reason to halt."""
        named = report.identify_slack_stragglers()["straggler_gpus_slack"]
        if not named:
            return
        scores = report.slack_scores()
        if self.slack_peer_groups:
            parts = [f"rank {rank} (its peer group {scores['ranks'][rank]['group']!r} waits "
                     f"{scores['ranks'][rank]['lead_us']:.0f} us per window for it)"
                     for rank in sorted(getattr(s, "rank", s) for s in named)]
            self.logger.warning("STRAGGLER DETECTION WARNING: Some GPUs' peer groups wait for them in their collectives "
                                "(slow host?): " + "; ".join(parts))
            return
        parts = [f"rank {rank} (the others wait {scores['ranks'][rank]['lead_us']:.0f} us per window for it)"
                 for rank in sorted(getattr(s, "rank", s) for s in named)]
        self.logger.warning("STRAGGLER DETECTION WARNING: The job waits for some GPUs in its collectives (slow host?): "
                            + "; ".join(parts) + f"; the typical rank spends {100 * scores['typical_share']:.1f} % of its "
                            "traced GPU time waiting")

    def _warn_off_pace(self, report) -> None:
        """One warning per report that names the GPUs that are a little slower than the job's median in nearly all of their
        kernels, with their pace and the microseconds spent above the median pace (``warn_if_off_pace``).  Never a reason to
        halt."""
        named = report.identify_pace_stragglers()["straggler_gpus_relative"]
        if not named:
            return
        ranks = report.pace_scores()["ranks"]
        parts = []
        for rank in sorted(getattr(s, "rank", s) for s in named):
            gpu = ranks[rank]["gpu"]
            parts.append(f"rank {rank} (pace {gpu['pace']:.3f}, slower in {gpu['slower']} of {gpu['columns']} kernels, "
                         f"excess_us={gpu['excess_us']:.0f})")
        if self.pace_peer_groups:
            self.logger.warning("STRAGGLER DETECTION WARNING: Some GPUs are off their peer group's pace, a little slower than "
                                "their group's median in nearly all of their kernels (degraded card?): " + "; ".join(parts))
            return
        self.logger.warning("STRAGGLER DETECTION WARNING: Some GPUs are a little slower in nearly all of their kernels "
                            "(degraded card?): " + "; ".join(parts))

    def _warn_node_off_pace(self, report) -> None:
        """One warning per report that names the nodes that are a little slower than the job's nodes in nearly all of their
        kernels, most of their GPUs agreeing, with their pace and how many of their GPUs are off pace
        (``warn_if_node_off_pace``).  Never a reason to halt."""
        named = report.identify_node_stragglers()["straggler_nodes"]
        if not named:
            return
        nodes = report.node_scores()["node_scores"]
        parts = []
        for label in sorted(named, key=str):
            d = nodes[label]
            parts.append(f"node {label} (pace {d['gpu']['pace']:.3f}, slower in {d['gpu']['slower']} of {d['gpu']['columns']} "
                         f"kernels, {d['members_off_pace']} of {d['members_rated']} GPUs off pace)")
        self.logger.warning("STRAGGLER DETECTION WARNING: Some nodes are a little slower in nearly all of their kernels on most "
                            "of their GPUs (host fault: cooling, power, host CPU?): " + "; ".join(parts))

    def _name_the_kernels(self, report, flagged) -> None:
        """Kernel attribution (``NVRX_KERNEL_ATTRIBUTION=N``, off by default: nothing is logged then): for every flagged GPU the
        kernels that carry its score's deficit, by name, with their share of it and the microseconds lost."""
        explain = getattr(report, "explain_gpu_scores", None)
        explained = explain() if explain is not None else {}
        if not explained:
            return
        for family, key in (("relative", "straggler_gpus_relative"), ("individual", "straggler_gpus_individual")):
            per_rank = explained.get(family, {})
            for rank in sorted(getattr(s, "rank", s) for s in flagged[key]):
                entry = per_rank.get(rank)
                if not entry or not entry["kernels"]:
                    continue
                top = ", ".join(f"{k['kernel']} (share {k['share']:.2f}, score {k['score']:.2f}, lost {k['lost_us']:.0f} us)"
                                for k in entry["kernels"] if k["lost_us"] > 0)
                self.logger.warning(f"STRAGGLER DETECTION WARNING: rank {rank} {family} GPU score deficit {entry['deficit']:.2f}, "
                                    f"top kernels: {top or 'none above the reference pace'}")

    def _telemetry_of_a_flagged_reporter(self, groups) -> None:
        # MI355X extra: when the reporting rank itself is flagged, say what ROCm SMI sees on its GPU (clock below
        # peak, hot junction, power) -- the first things to rule out for a slow GPU
        det = straggler.Detector
        me = getattr(det.reporter, "rank", None) if det.initialized else None
        if me is not None and any(getattr(s, "rank", None) == me for group in groups for s in group):
            self.logger.warning(f"rank {me}: {det.gpu_telemetry_line()}")

    @staticmethod
    def _ranking(rank_to_score, rank_to_node, num_best=3, num_worst=3) -> str:
        """Worst ``num_worst`` and best ``num_best`` ranks (all of them if there are no more than that), one
        ``Rank= Node= Score=`` line each; ties go by rank, as sorting (score, rank) pairs gives them."""
        ascending = sorted((score, rank) for rank, score in rank_to_score.items())
        total = len(ascending)

        def lines(pairs):
            return "".join(f"  Rank={rank} Node={rank_to_node[rank]} Score={score:.2f}\n" for score, rank in pairs)

        if total <= num_best + num_worst:
            return lines(ascending)
        return (f" Worst performing {num_worst}/{total} ranks:\n" + lines(ascending[:num_worst])
                + f" Best performing {num_best}/{total} ranks:\n" + lines(reversed(ascending[-num_best:])))

    # the reference's name for the same text (a static helper some users call directly)
    _format_gpu_scores = _ranking

    def _log_extremes(self, pl_module, rank_to_score, prefix) -> None:
        """min / median / max of one score family to every PTL logger; NaN when the family is empty."""
        stats = dict.fromkeys(("min", "median", "max"), float("nan"))
        if rank_to_score:
            t = torch.tensor(list(rank_to_score.values()), dtype=torch.float32)
            stats = {"min": torch.min(t).item(), "median": torch.median(t).item(), "max": torch.max(t).item()}
        try:
            pl_module.log_dict({f"{prefix}/{k}": v for k, v in stats.items()}, logger=True, batch_size=1, rank_zero_only=True)
        except Exception as e:  # logging must never take training down
            self.logger.error(f"Failed to log GPU performance scores: {e}")

    # ---- stopping the job -----------------------------------------------------------------------------
    def _decision_of_rank0(self, flag) -> bool:
        """Rank 0's verdict on every rank (a broadcast on the process group's own device; no group: the flag)."""
        if not (torch.distributed.is_available() and torch.distributed.is_initialized()):
            return bool(flag)
        t = torch.tensor([1.0 if flag else 0.0], dtype=torch.float32, device=dist_utils.get_device_for_backend(None))
        torch.distributed.broadcast(t, 0)
        return bool(t.item() > 0)

    def _halt(self, trainer) -> None:
        self.logger.error("Detected stragglers. Terminating training...")
        trainer.should_stop = True
        checkpointing = trainer.checkpoint_callback
        if not checkpointing:
            return
        # a last checkpoint, an asynchronous one awaited, then out
        checkpointing._save_last_checkpoint(trainer, checkpointing._monitor_candidates(trainer))
        finalize = getattr(trainer.strategy.checkpoint_io, "maybe_finalize_save_checkpoint", None)
        if finalize is not None:
            self.logger.info("Async checkpointing detected, waiting for it to complete...")
            finalize(blocking=True)
        sys.exit(1)
