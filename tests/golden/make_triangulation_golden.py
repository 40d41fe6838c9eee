"""Writes tests/golden/triangulation/door_tracks2d.npz from the reference's tests/data/tracks2d_door.pickle.

    python tests/golden/make_triangulation_golden.py /path/to/gtsfm

The pickle holds a list of gtsfm.common.sfm_track.SfmTrack2d (8,824 tracks, 46,493 measurements, lengths 2-12). It is
decoded with a restricted unpickler that maps gtsfm.common.sfm_track onto this package's classes and admits nothing
else but numpy's array reconstruction, then re-encoded as a CSR: offsets int32, image int32, uv float32. Every stored
uv is exactly a float32 value (checked), so nothing is lost. The reference is read only here, at generation time.
"""
import os
import pickle
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from gtsfm_amd.common import sfm_track  # noqa: E402

_ALLOWED = {
    ("gtsfm.common.sfm_track", "SfmTrack2d"): sfm_track.SfmTrack2d,
    ("gtsfm.common.sfm_track", "SfmMeasurement"): sfm_track.SfmMeasurement,
}
_NUMPY_OK = {"_reconstruct", "ndarray", "dtype", "scalar"}


class _Restricted(pickle.Unpickler):
    def find_class(self, module, name):
        if (module, name) in _ALLOWED:
            return _ALLOWED[(module, name)]
        if module.split(".")[0] == "numpy" and name in _NUMPY_OK:
            return super().find_class(module, name)
        raise pickle.UnpicklingError(f"{module}.{name} is not allowed in the tracks pickle")


def main(reference_root: str) -> None:
    with open(os.path.join(reference_root, "tests", "data", "tracks2d_door.pickle"), "rb") as f:
        tracks = _Restricted(f).load()
    lens = [t.number_measurements() for t in tracks]
    offsets = np.zeros(len(tracks) + 1, np.int32)
    np.cumsum(lens, out=offsets[1:])
    image = np.array([m.i for t in tracks for m in t.measurements], np.int32)
    uv64 = np.array([np.asarray(m.uv, np.float64) for t in tracks for m in t.measurements]).reshape(-1, 2)
    uv = uv64.astype(np.float32)
    assert np.array_equal(uv.astype(np.float64), uv64), "a stored uv is not a float32 value"
    out = os.path.join(HERE, "triangulation", "door_tracks2d.npz")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    np.savez_compressed(out, offsets=offsets, image=image, uv=uv)
    print(f"{out}: {len(tracks)} tracks, {len(image)} measurements, lengths {min(lens)}-{max(lens)}, "
          f"{os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
