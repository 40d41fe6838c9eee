"""Base class for track estimation (gtsfm/data_association/tracks_estimator_base.py)."""
import abc
from typing import Dict, List, Tuple

import numpy as np

from gtsfm_amd.common.keypoints import Keypoints
from gtsfm_amd.common.sfm_track import SfmTrack2d


class TracksEstimatorBase(metaclass=abc.ABCMeta):
    """Turns pairwise feature correspondences into 2D tracks."""

    @abc.abstractmethod
    def run(self, matches_dict: Dict[Tuple[int, int], np.ndarray], keypoints_list: List[Keypoints]) -> List[SfmTrack2d]:
        """matches_dict: (i1, i2) -> (K, 2) rows (k1, k2) of keypoint indices into keypoints_list[i1] / [i2].
        Returns every valid track the matches generate."""
