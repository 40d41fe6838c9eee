"""2D tracks: the measurements of one scene point across images, with the reference's API
(gtsfm/common/sfm_track.py:17-112), so that code written against the reference's SfmTrack2d reads these unchanged.
"""
from typing import Iterable, List, NamedTuple, Tuple

import numpy as np

from gtsfm_amd.common import geometry


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


if geometry.HAVE_GTSAM:  # pragma: no cover - exercised only where gtsam is installed
    import gtsam  # type: ignore

    SfmTrack = gtsam.SfmTrack
else:

    class SfmTrack:  # type: ignore[no-redef]
        """Stand-in for gtsam.SfmTrack: a 3D point and its (camera index, uv) measurements, with the accessors the
        reference's data association uses."""

        def __init__(self, point3=(0.0, 0.0, 0.0)):
            self._p = np.asarray(point3, dtype=np.float64).reshape(3).copy()
            self._measurements: List[Tuple[int, np.ndarray]] = []

        def point3(self) -> np.ndarray:
            return self._p.copy()

        def numberMeasurements(self) -> int:
            return len(self._measurements)

        def measurement(self, idx: int) -> Tuple[int, np.ndarray]:
            return self._measurements[idx]

        def addMeasurement(self, idx: int, uv) -> None:
            self._measurements.append((int(idx), np.asarray(uv, dtype=np.float64).reshape(2).copy()))

        def __reduce__(self):
            return (_rebuild_sfm_track, (self._p, self._measurements))


def _rebuild_sfm_track(point3, measurements):
    track = SfmTrack(point3)
    for i, uv in measurements:
        track.addMeasurement(i, uv)
    return track
