"""TriangulationOptions, the sampling modes and the exit codes (reference
gtsfm/data_association/point3d_initializer.py:36-114).

The two-view bundle adjustment reads `mode` (which must be NO_RANSAC there: the two-view estimator's configuration,
sift_front_end.yaml), `reproj_error_threshold` (default inf, "no filtering unless specified") and
`min_triangulation_angle` (default 0: no rejection). The RANSAC fields feed num_ransac_hypotheses(), which
gtsfm_amd/data_association/point3d_initializer.py passes to the track triangulation kernel.
"""
import math
import sys
from enum import Enum
from typing import NamedTuple


NUM_SAMPLES_PER_RANSAC_HYPOTHESIS = 2


class TriangulationExitCode(Enum):
    """Exit codes of a track's triangulation (point3d_initializer.py:36-45); the kernel writes these values."""

    SUCCESS = 0  # the 3D point was estimated
    CHEIRALITY_FAILURE = 1  # triangulatePoint3 failed (cheirality, or a rank-deficient system)
    INLIERS_UNDERCONSTRAINED = 2  # fewer than two inlier measurements
    POSES_UNDERCONSTRAINED = 3  # fewer than two inlier measurements in cameras with a pose
    EXCEEDS_REPROJ_THRESH = 4  # an inlier's reprojection error is not below the threshold
    LOW_TRIANGULATION_ANGLE = 5  # the largest triangulation angle is below the minimum


class TriangulationSamplingMode(str, Enum):
    NO_RANSAC = "NO_RANSAC"
    RANSAC_SAMPLE_UNIFORM = "RANSAC_SAMPLE_UNIFORM"
    RANSAC_SAMPLE_BIASED_BASELINE = "RANSAC_SAMPLE_BIASED_BASELINE"
    RANSAC_TOPK_BASELINES = "RANSAC_TOPK_BASELINES"


class TriangulationOptions(NamedTuple):
    mode: TriangulationSamplingMode
    reproj_error_threshold: float = math.inf
    min_triangulation_angle: float = 0.0
    min_inlier_ratio: float = 0.1
    confidence: float = 0.9999
    dyn_num_hypotheses_multiplier: float = 3.0
    min_num_hypotheses: int = 0
    max_num_hypotheses: int = sys.maxsize

    def __check_ransac_params(self) -> None:
        assert self.reproj_error_threshold > 0
        assert 0 < self.min_inlier_ratio < 1
        assert 0 < self.confidence < 1
        assert self.dyn_num_hypotheses_multiplier > 0
        assert 0 <= self.min_num_hypotheses < self.max_num_hypotheses

    def num_ransac_hypotheses(self) -> int:
        """The number of hypotheses (point3d_initializer.py:102-114): log(1 - confidence) / log(1 - ratio^2) times the
        multiplier, clamped to [min_num_hypotheses, max_num_hypotheses]; 2749 with the defaults."""
        self.__check_ransac_params()
        dyn_num_hypotheses = int(
            (math.log(1 - self.confidence) / math.log(1 - self.min_inlier_ratio ** NUM_SAMPLES_PER_RANSAC_HYPOTHESIS))
            * self.dyn_num_hypotheses_multiplier
        )
        return max(min(self.max_num_hypotheses, dyn_num_hypotheses), self.min_num_hypotheses)
