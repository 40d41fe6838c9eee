"""Cycle-consistent rotation view-graph filter on the MI355X.

Drop-in for gtsfm/view_graph_estimator/cycle_consistent_rotation_estimator.py:49-152: every 3-cycle of relative
rotations is composed (geometry_comparisons.py:355-370), the angle of the composed rotation is the cycle error, each
edge aggregates the errors of the triplets it is part of by min or median, and an edge stays in the view graph when
that aggregate is below the threshold. The reference loops over the triplets in Python; here one
gtsfm_viewgraph_cycle_filter launch (libgtsfm_hip.so) does all of it, one workgroup per edge.
"""
import logging
from enum import Enum
from pathlib import Path
from typing import Any, Dict, List, Optional, Set, Tuple, Union

import numpy as np
import torch

from gtsfm_amd import device, native
from gtsfm_amd.common import geometry, upload
from gtsfm_amd.view_graph_estimator.view_graph_estimator_base import ViewGraphEstimatorBase

logger = logging.getLogger(__name__)

ERROR_THRESHOLD = 7.0  # degrees (cycle_consistent_rotation_estimator.py:26)

ArrayLike = Union[np.ndarray, torch.Tensor]


class EdgeErrorAggregationCriterion(str, Enum):
    """How an edge summarises the cycle errors of its triplets (cycle_consistent_rotation_estimator.py:32-46):
    MIN_EDGE_ERROR accepts an edge that is in ANY low-error cycle; MEDIAN_EDGE_ERROR wants half of them to be."""

    MIN_EDGE_ERROR = "MIN_EDGE_ERROR"
    MEDIAN_EDGE_ERROR = "MEDIAN_EDGE_ERROR"


_CRITERION = {
    EdgeErrorAggregationCriterion.MIN_EDGE_ERROR: native.GTSFM_VG_MIN_EDGE_ERROR,
    EdgeErrorAggregationCriterion.MEDIAN_EDGE_ERROR: native.GTSFM_VG_MEDIAN_EDGE_ERROR,
}


class CycleConsistentRotationViewGraphEstimator(ViewGraphEstimatorBase):
    """Keeps the two-view edges whose aggregated rotation-cycle error is below error_threshold degrees."""

    def __init__(self, edge_error_aggregation_criterion: EdgeErrorAggregationCriterion,
                 error_threshold: float = ERROR_THRESHOLD) -> None:
        self._edge_error_aggregation_criterion = EdgeErrorAggregationCriterion(edge_error_aggregation_criterion)
        self._error_threshold = float(error_threshold)

    def run_arrays(self, pairs: ArrayLike, R: ArrayLike, valid: Optional[ArrayLike] = None,
                   num_images: Optional[int] = None) -> Tuple[ArrayLike, ArrayLike, ArrayLike]:
        """The filter on arrays: pairs (P, 2) int with i1 < i2, R (P, 3, 3) float64 i2Ri1, valid (P,) bool or None:
        the layout of HostResults.pairs / .R with valid = (status == 0) & isp_ok. Pairs may come in any order.

        Returns (keep (P,) bool, agg_error_deg (P,) float64, n_triplets (P,) int32) in input order, of the kind of
        `pairs`: numpy in gives numpy out, a torch tensor in gives torch tensors on that tensor's device (a CPU tensor
        is copied to the GPU and the results back, like numpy). With `pairs` on the GPU and num_images given (every
        index < num_images) nothing is copied to the host or synchronised; num_images None reads the largest index of
        pairs back, which is one host synchronisation.
        An invalid pair, or one with i1 >= i2, is no edge of the graph: keep False, NaN, 0."""
        is_tensor = isinstance(pairs, torch.Tensor)
        dev = upload.cuda_device(pairs)
        pairs_d = upload.to_device(pairs, dev, torch.int32, (-1, 2))
        P = pairs_d.shape[0]
        R_d = upload.to_device(R, dev, torch.float64, (P, 9))
        valid_d = None if valid is None else upload.mask_to_device(valid, dev, P)
        if num_images is None:
            num_images = int(pairs_d.max().item()) + 1 if P else 0
        keep, agg, n_trip, _ = device.viewgraph_cycle_filter(
            pairs_d, R_d, valid_d, int(num_images), _CRITERION[self._edge_error_aggregation_criterion],
            self._error_threshold, want_total=False)
        keep = keep.bool()
        if is_tensor:
            return keep.to(pairs.device), agg.to(pairs.device), n_trip.to(pairs.device)
        return keep.cpu().numpy(), agg.cpu().numpy(), n_trip.cpu().numpy()

    def run(
        self,
        i2Ri1_dict: Dict[Tuple[int, int], Any],
        i2Ui1_dict: Dict[Tuple[int, int], Any],
        calibrations: List[Any],
        corr_idxs_i1i2: Dict[Tuple[int, int], np.ndarray],
        keypoints: List[Any],
        two_view_reports: Dict[Tuple[int, int], Any],
        output_dir: Optional[Path] = None,
    ) -> Set[Tuple[int, int]]:
        """The reference's run(): only i2Ri1_dict is read (values: 3x3 ndarrays or Rot3-like objects with .matrix());
        output_dir is accepted and ignored (no plots). Pairs with i1 >= i2 or a None rotation are skipped."""
        edges: List[Tuple[int, int]] = []
        mats: List[np.ndarray] = []
        for (i1, i2), i2Ri1 in i2Ri1_dict.items():
            if i1 >= i2:
                logger.error("cycle consistency: edge (%d, %d) is not ordered i1 < i2, skipped", i1, i2)
                continue
            if i2Ri1 is None:
                continue
            edges.append((int(i1), int(i2)))
            mats.append(geometry.rotation_matrix(i2Ri1).reshape(3, 3))
        if not edges:
            return set()
        order = sorted(range(len(edges)), key=edges.__getitem__)  # (i1, i2) order: the kernel's cache-friendly one
        pairs = np.array([edges[k] for k in order], dtype=np.int32)
        keep, _, _ = self.run_arrays(pairs, np.stack([mats[k] for k in order]))
        view_graph_edges = {edges[order[k]] for k in np.flatnonzero(np.asarray(keep))}
        logger.info("cycle consistency: %d of %d edges kept", len(view_graph_edges), len(edges))
        return view_graph_edges
