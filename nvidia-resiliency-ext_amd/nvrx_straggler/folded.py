"""Several logical ranks per GPU: the harness used to run a whole R-rank job on fewer GPUs.

BASELINE.json quotes the metric on 8 ranks x 64 sections x 10 000 samples and asks for it at 1, 2, 4
and 8 GPUs.  With fewer than 8 GPUs each process holds ``R / world_size`` logical ranks' timing
matrices in one set of device rings (``local_ranks`` of ``nvrx_ctx_create``); the statistics kernel
then covers ``local_ranks * S`` rows per launch, the all-gather carries ``local_ranks`` exchange rows
per process, and the score kernel sees the same ``[R, L]`` table as an 8-GPU run.  Production use is
always one logical rank per GPU (``Detector``); this class exists for ``bench.py`` and the
full-size parity tests.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import _native, dist_utils
from .backend import get_backend
from .reporting import ReportGenerator


class FoldedJob:
    def __init__(self, total_ranks: int = 8, section_names: Optional[Sequence[str]] = None, sections: int = 64,
                 ring_cap: int = 8192, scores_to_compute=("relative_perf_scores", "individual_perf_scores"),
                 gather_on_rank0: bool = True, pg=None, node_name: str = "node", kernel_attribution: int = 0,
                 tail_quantile: float = 0.0, robust_scores: bool = False, asynchronous: bool = False,
                 onset_detection: bool = False, onset_min_segment: float = 0.05, onset_min_strength: float = 0.5,
                 period_detection: bool = False, period_max: int = 1024, period_min_strength: float = 0.5,
                 episode_detection: bool = False, episode_min_length: float = 0.005, episode_min_strength: float = 0.5,
                 score_history: int = 0, persistence_min_reports: int = 3, persistence_thresholds=None,
                 score_trends: bool = False, trend_min_reports: int = 6, trend_min_tau: float = 0.6, trend_horizon=None,
                 collective_slack: bool = False, slack_min_ranks: int = 4, slack_min_share: float = 0.05,
                 slack_max_ratio: float = 0.25, kernel_names: Sequence[str] = (), peer_groups=None, peer_min_ranks: int = 2,
                 pace_scores: bool = False, pace_min_ranks: int = 4, pace_min_columns: int = 8, pace_min_effect: float = 0.03,
                 pace_min_breadth: float = 0.9, pace_peer_groups: bool = False, node_scores: bool = False, node_groups=None,
                 node_min_members: int = 2, node_min_nodes: int = 3, node_min_columns: int = 8, node_min_effect: float = 0.03,
                 node_min_breadth: float = 0.9, node_min_agree: float = 0.75, work_groups: bool = False,
                 work_count_tol: float = 0.25, work_max_unlike: float = 0.1, peer_history: int = 0,
                 peer_persistence_min_reports: int = 3, peer_persistence_thresholds=None, peer_trends: bool = False,
                 slack_peer_groups: bool = False, row_peer_groups: bool = False):
        world = dist_utils.get_world_size(pg)
        if total_ranks % world:
            raise ValueError(f"total_ranks {total_ranks} must be a multiple of the world size {world}")
        self.total_ranks = total_ranks
        self.local_ranks = total_ranks // world
        self.world_rank = dist_utils.get_rank(pg)
        self.section_names = list(section_names) if section_names is not None else [f"section_{s:03d}" for s in range(sections)]
        self.backend = get_backend()
        self.kernel_names = list(kernel_names)  # per-kernel rows next to the sections (``load_kernels``); none by default
        self.rings = self.backend.make_rings(self.local_ranks, len(self.section_names) + len(self.kernel_names), ring_cap)
        self.ring_cap = ring_cap
        self.reporter = ReportGenerator(list(scores_to_compute), gather_on_rank0=gather_on_rank0, pg=pg, node_name=node_name,
                                        kernel_attribution=kernel_attribution, tail_quantile=tail_quantile,
                                        robust_scores=robust_scores, asynchronous=asynchronous,
                                        onset_detection=onset_detection, onset_min_segment=onset_min_segment,
                                        onset_min_strength=onset_min_strength, period_detection=period_detection,
                                        period_max=period_max, period_min_strength=period_min_strength,
                                        episode_detection=episode_detection, episode_min_length=episode_min_length,
                                        episode_min_strength=episode_min_strength, score_history=score_history,
                                        persistence_min_reports=persistence_min_reports,
                                        persistence_thresholds=persistence_thresholds, score_trends=score_trends,
                                        trend_min_reports=trend_min_reports, trend_min_tau=trend_min_tau,
                                        trend_horizon=trend_horizon, collective_slack=collective_slack,
                                        slack_min_ranks=slack_min_ranks, slack_min_share=slack_min_share,
                                        slack_max_ratio=slack_max_ratio, peer_groups=peer_groups,
                                        peer_min_ranks=peer_min_ranks, pace_scores=pace_scores,
                                        pace_min_ranks=pace_min_ranks, pace_min_columns=pace_min_columns,
                                        pace_min_effect=pace_min_effect, pace_min_breadth=pace_min_breadth,
                                        **({"pace_peer_groups": True} if pace_peer_groups else {}),
                                        **({"slack_peer_groups": True} if slack_peer_groups else {}),
                                        **({"row_peer_groups": True} if row_peer_groups else {}),
                                        **({"peer_history": peer_history,
                                            "peer_persistence_min_reports": peer_persistence_min_reports,
                                            "peer_persistence_thresholds": peer_persistence_thresholds,
                                            "peer_trends": peer_trends} if peer_history or peer_trends else {}),
                                        **({"node_scores": True, "node_groups": node_groups,
                                            "node_min_members": node_min_members, "node_min_nodes": node_min_nodes,
                                            "node_min_columns": node_min_columns, "node_min_effect": node_min_effect,
                                            "node_min_breadth": node_min_breadth, "node_min_agree": node_min_agree}
                                           if node_scores else {}),
                                        **({"work_groups": bool(work_groups), "work_count_tol": work_count_tol,
                                            "work_max_unlike": work_max_unlike}
                                           if work_groups or (isinstance(peer_groups, str) and peer_groups == "auto") else {}))
        self.rows = {name: self.rings.row_for(_native.KIND_SECTION, name) for name in self.section_names}
        # (the same object every report so the reporter's cached plan stays valid)
        self._no_kernel_rows = {name: self.rings.row_for(_native.KIND_KERNEL, name) for name in self.kernel_names}

    def logical_ranks(self):
        """Global logical ranks held by this process."""
        return range(self.world_rank * self.local_ranks, (self.world_rank + 1) * self.local_ranks)

    def load(self, lr: int, samples) -> None:
        """Append ``samples`` ([S, n] f32, host array or device tensor) to logical rank ``lr``'s rings."""
        if isinstance(samples, np.ndarray):
            samples = torch.from_numpy(np.ascontiguousarray(samples, dtype=np.float32)).to(self.backend.device)
        self.backend.synchronize()
        torch.cuda.current_stream().synchronize()
        rows = [self.rows[name] for name in self.section_names]
        if rows == list(range(rows[0], rows[0] + len(rows))) and samples.dim() == 2 and samples.stride(1) == 1:
            self.rings.push_device_rows(rows[0], samples, lr=lr)     # the whole matrix in one call
        else:
            for s, row in enumerate(rows):
                self.rings.push_device(row, samples[s].contiguous(), lr=lr)
        self.backend.synchronize()

    def load_kernels(self, lr: int, samples) -> None:
        """Append ``samples`` ([len(kernel_names), n] f32 host array: microseconds per call) to logical rank ``lr``'s kernel
        rows, as the per-kernel tracer would."""
        for name, values in zip(self.kernel_names, samples):
            self.rings.push_many(self._no_kernel_rows[name], values, lr=lr)

    def rearm(self, n: int) -> None:
        """Declare every row holds ``n`` resident samples again (after a report emptied the rings)."""
        self.rings.set_count_all(n)

    def report(self, reset: bool = True):
        # (reset: the generator empties the rings itself, while the GPU runs where the report allows it)
        return self.reporter.generate_report_from_rings(self.rings, self.rows, self._no_kernel_rows,
                                                        local_ranks=self.local_ranks, reset_rings=reset)

    def close(self) -> None:
        self.reporter.close()
        self.rings.close()
