"""Base class of the translation averaging plugins (gtsfm/averaging/translation/translation_averaging_base.py:23-80).
create_computation_graph (Dask) stays with the reference."""
import abc
from typing import Dict, List, Optional, Tuple


class TranslationAveragingBase(metaclass=abc.ABCMeta):
    """Estimates global camera positions from relative unit translations and global rotations."""

    def __init__(self, robust_measurement_noise: bool = True) -> None:
        self._robust_measurement_noise = robust_measurement_noise

    @abc.abstractmethod
    def run_translation_averaging(self, num_images: int, i2Ui1_dict: Dict[Tuple[int, int], Optional[object]],
                                  wRi_list: List[Optional[object]], tracks_2d=None, intrinsics=None,
                                  absolute_pose_priors=(), i2Ti1_priors=None, scale_factor: float = 1.0,
                                  gt_wTi_list=()) -> Tuple[List[Optional[object]], Optional[dict]]:
        """Returns the global poses wTi (None where no position could be computed) and a metrics dict."""
