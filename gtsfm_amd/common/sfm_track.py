"""2D tracks: the measurements of one scene point across images, with the reference's API
(gtsfm/common/sfm_track.py:17-112), so that code written against the reference's SfmTrack2d reads these unchanged.
"""
from typing import Iterable, List, NamedTuple

import numpy as np


class SfmMeasurement(NamedTuple):
    """One detection: i is the camera (image) index, uv its (2,) pixel position."""

    i: int
    uv: np.ndarray

    def __eq__(self, other: object) -> bool:
        """Same camera and the same position up to np.allclose's default tolerance."""
        return isinstance(other, SfmMeasurement) and self.i == other.i and bool(np.allclose(self.uv, other.uv))

    def __ne__(self, other: object) -> bool:
        return not self.__eq__(other)


class SfmTrack2d(NamedTuple):
    """The 2D measurements of a single 3D point (a gtsam.SfmTrack before its point is triangulated)."""

    measurements: List[SfmMeasurement]

    def number_measurements(self) -> int:
        return len(self.measurements)

    def measurement(self, idx: int) -> SfmMeasurement:
        return self.measurements[idx]

    def select_subset(self, idxs: List[int]) -> "SfmTrack2d":
        """The track made of measurements idxs, in that order; every index must exist."""
        return SfmTrack2d([self.measurements[j] for j in idxs])

    def select_for_cameras(self, camera_idxs: Iterable[int]) -> "SfmTrack2d":
        """The track restricted to the given cameras; cameras without a measurement here are simply absent."""
        wanted = set(camera_idxs)
        return SfmTrack2d([m for m in self.measurements if m.i in wanted])

    def validate_unique_cameras(self) -> bool:
        """True iff no camera contributes two measurements."""
        cams = [m.i for m in self.measurements]
        return len(cams) == len(set(cams))

    def __eq__(self, other: object) -> bool:
        """Equal measurement counts, and every measurement of this track occurs in the other, in any order."""
        if not isinstance(other, SfmTrack2d) or len(self.measurements) != len(other.measurements):
            return False
        return all(any(m == o for o in other.measurements) for m in self.measurements)

    def __ne__(self, other: object) -> bool:
        return not self.__eq__(other)
