"""Base class of the rotation averaging plugins (gtsfm/averaging/rotation/rotation_averaging_base.py).
create_computation_graph (Dask) and evaluate (ground-truth metrics) stay with the reference."""
import abc
from typing import Dict, List, Optional, Tuple


class RotationAveragingBase(metaclass=abc.ABCMeta):
    """Estimates global camera rotations from relative ones."""

    @abc.abstractmethod
    def run_rotation_averaging(self, num_images: int, i2Ri1_dict: Dict[Tuple[int, int], Optional[object]],
                               i1Ti2_priors: Dict[Tuple[int, int], object]) -> List[Optional[object]]:
        """Returns the global rotations wRi, None where none could be computed."""
