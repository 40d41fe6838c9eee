"""Base class for view-graph estimation.

Drop-in for gtsfm/view_graph_estimator/view_graph_estimator_base.py:37-341 without Dask: estimate() runs eagerly what
create_computation_graph (:251-341) wires as delayed tasks, as run_two_view_estimator_as_futures does in this project.
Metrics and plots (compute_metrics, :159-249) stay with the reference.
"""
import abc
import logging
from pathlib import Path
from typing import Any, Dict, List, Optional, Set, Tuple

import numpy as np

logger = logging.getLogger(__name__)

EdgeDicts = Tuple[Dict[Tuple[int, int], Any], Dict[Tuple[int, int], Any], Dict[Tuple[int, int], np.ndarray],
                  Dict[Tuple[int, int], Any]]


class ViewGraphEstimatorBase(metaclass=abc.ABCMeta):
    """Aggregates two-view estimates into a view graph, possibly filtering them."""

    @abc.abstractmethod
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
        """Edges of the view graph, a subset of the input pairs. The input dicts are valid: i1 < i2 and neither
        i2Ri1 nor i2Ui1 is None (view_graph_estimator_base.py:64-89)."""

    def _get_valid_input_edges(self, i2Ri1_dict: Dict[Tuple[int, int], Any],
                               i2Ui1_dict: Dict[Tuple[int, int], Any]) -> List[Tuple[int, int]]:
        """The keys of i2Ri1_dict that are usable edges, in dict order: ordered i1 < i2, with a rotation and a unit
        translation that both exist (view_graph_estimator_base.py:91-119). A misordered key, or a rotation without a
        translation entry, is an upstream bug and is logged; a None value is an edge dropped earlier and is not."""
        misordered = [key for key in i2Ri1_dict if key[0] >= key[1]]
        orphaned = [key for key, rot in i2Ri1_dict.items()
                    if key[0] < key[1] and rot is not None and key not in i2Ui1_dict]
        for key in misordered:
            logger.error("view graph: edge %s is not ordered i1 < i2, skipped", key)
        for key in orphaned:
            logger.error("view graph: edge %s has a rotation but no unit translation, skipped", key)
        return [key for key, rot in i2Ri1_dict.items()
                if key[0] < key[1] and rot is not None and i2Ui1_dict.get(key) is not None]

    def _filter_with_edges(self, i2Ri1_dict: Dict[Tuple[int, int], Any], i2Ui1_dict: Dict[Tuple[int, int], Any],
                           corr_idxs_i1i2: Dict[Tuple[int, int], np.ndarray],
                           two_view_reports: Dict[Tuple[int, int], Any], edges_to_select) -> EdgeDicts:
        """The four two-view dicts restricted to edges_to_select (view_graph_estimator_base.py:121-157); a selected
        edge missing from one of them is a KeyError, as in the reference."""
        selected = list(edges_to_select)
        sources = (i2Ri1_dict, i2Ui1_dict, corr_idxs_i1i2, two_view_reports)
        return tuple({key: source[key] for key in selected} for source in sources)

    def estimate(
        self,
        i2Ri1_dict: Dict[Tuple[int, int], Any],
        i2Ui1_dict: Dict[Tuple[int, int], Any],
        calibrations: List[Any],
        corr_idxs_i1i2: Dict[Tuple[int, int], np.ndarray],
        keypoints: List[Any],
        two_view_reports: Dict[Tuple[int, int], Any],
        debug_output_dir: Optional[Path] = None,
    ) -> EdgeDicts:
        """Drops the invalid input edges, runs run() on the rest and returns (i2Ri1, i2Ui1, corr_idxs_i1i2,
        two_view_reports) restricted to the view graph's edges: create_computation_graph's first four outputs."""
        valid_edges = self._get_valid_input_edges(i2Ri1_dict, i2Ui1_dict)
        valid = self._filter_with_edges(i2Ri1_dict, i2Ui1_dict, corr_idxs_i1i2, two_view_reports, valid_edges)
        view_graph_edges = self.run(valid[0], valid[1], calibrations, valid[2], keypoints, valid[3],
                                    output_dir=debug_output_dir)
        return self._filter_with_edges(*valid, view_graph_edges)
