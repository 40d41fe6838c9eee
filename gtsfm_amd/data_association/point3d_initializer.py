"""3D landmarks from 2D tracks at known camera poses, on the MI355X.

Drop-in for gtsfm/data_association/point3d_initializer.py:117-380: Point3dInitializer.triangulate(track_2d) keeps the
reference's return conventions, and triangulate_arrays() is the batch form that triangulates every track of a
Tracks2d CSR in one gtsfm_triangulate_tracks call (libgtsfm_hip.so) where the reference makes one Python call per
track with up to num_ransac_hypotheses() gtsam.triangulatePoint3 calls each. Semantics and the two stated deviations
(the hypothesis subset is a keyed pseudo-random choice instead of np.random.choice, equal hypotheses are ordered by pair
index) are in include/gtsfm_hip.h. RANSAC_SAMPLE_BIASED_BASELINE is not built and raises NotImplementedError.
"""
from typing import Dict, NamedTuple, Optional, Tuple, Union

import numpy as np
import torch

from gtsfm_amd import device, native
from gtsfm_amd.common import geometry, upload
from gtsfm_amd.common.sfm_track import SfmTrack, SfmTrack2d
from gtsfm_amd.data_association.dsf_tracks_estimator import Tracks2d
from gtsfm_amd.frontend.triangulation_options import (  # noqa: F401  (re-exported, as the reference module has them)
    TriangulationExitCode,
    TriangulationOptions,
    TriangulationSamplingMode,
)

ArrayLike = Union[np.ndarray, torch.Tensor]
DeviceCameras = Tuple[torch.Tensor, torch.Tensor, torch.Tensor, Optional[torch.Tensor]]

MODE_TO_NATIVE = {
    TriangulationSamplingMode.NO_RANSAC: native.GTSFM_TRI_NO_RANSAC,
    TriangulationSamplingMode.RANSAC_SAMPLE_UNIFORM: native.GTSFM_TRI_RANSAC_SAMPLE_UNIFORM,
    TriangulationSamplingMode.RANSAC_SAMPLE_BIASED_BASELINE: native.GTSFM_TRI_RANSAC_SAMPLE_BIASED_BASELINE,
    TriangulationSamplingMode.RANSAC_TOPK_BASELINES: native.GTSFM_TRI_RANSAC_TOPK_BASELINES,
}


class Triangulated(NamedTuple):
    """Per-track results as arrays (numpy or torch, as the tracks given): exit_code (T,) int32
    (TriangulationExitCode values), point (T, 3) float64 (NaN unless the final triangulation succeeded), avg_err (T,)
    float64 (NaN for exits 1-3), inlier (n_meas,) uint8 parallel to the tracks' measurements, stats (8,) int64 in the
    order of native.TRI_STATS_FIELDS."""

    exit_code: ArrayLike
    point: ArrayLike
    avg_err: ArrayLike
    inlier: ArrayLike
    stats: ArrayLike


class CameraArrays(NamedTuple):
    wRc: np.ndarray  # (n_img, 3, 3)
    wtc: np.ndarray  # (n_img, 3)
    intrinsics: np.ndarray  # (n_img, 3): f, u0, v0
    valid: np.ndarray  # (n_img,) uint8


def camera_arrays(track_camera_dict: Dict[int, object], num_images: Optional[int] = None) -> CameraArrays:
    """The cameras of a dict {image index: camera or None} as arrays indexed by image (missing / None: valid = 0)."""
    keys = [int(i) for i in track_camera_dict]
    n = max(keys) + 1 if num_images is None else int(num_images)
    wRc = np.tile(np.eye(3), (n, 1, 1))
    wtc = np.zeros((n, 3))
    intr = np.tile(np.array([1.0, 0.0, 0.0]), (n, 1))
    valid = np.zeros(n, np.uint8)
    for i, cam in track_camera_dict.items():
        if cam is None or not 0 <= int(i) < n:
            continue
        wRc[i], wtc[i] = geometry.camera_pose(cam)
        intr[i] = geometry.calibration_params(cam.calibration())
        valid[i] = 1
    return CameraArrays(wRc, wtc, intr, valid)


class Point3dInitializer:
    """Initialises landmark points by triangulation, with or without RANSAC over the track's measurement pairs."""

    def __init__(self, track_camera_dict: Union[Dict[int, object], DeviceCameras], options: TriangulationOptions,
                 seed: int = 0) -> None:
        """track_camera_dict: {image index: camera or None}, or the tuple (wRc (n_img, 3, 3), wtc (n_img, 3),
        intrinsics (n_img, 3) float64, cam_valid (n_img,) uint8) of device tensors that
        BundleAdjustmentOptimizer.run_ba_arrays takes too; the tuple is used as it is, with no host copy."""
        self.track_camera_dict = track_camera_dict
        self.options = options
        self.seed = int(seed)
        if not isinstance(track_camera_dict, dict):
            self._cams = None
            self._cams_dev = tuple(track_camera_dict)
            return
        if len(track_camera_dict) == 0:
            raise ValueError("No camera positions were estimated, so triangulation is not feasible.")
        self._cams = camera_arrays(track_camera_dict)
        self._cams_dev = None

    def _device_cameras(self, dev: torch.device):
        if self._cams is None:
            return self._cams_dev
        if self._cams_dev is None or self._cams_dev[0].device != dev:
            c = self._cams
            self._cams_dev = tuple(upload.to_device(a, dev) for a in (c.wRc, c.wtc, c.intrinsics, c.valid))
        return self._cams_dev

    def _n_hyp(self) -> int:
        if self.options.mode == TriangulationSamplingMode.NO_RANSAC:
            return 0
        return min(self.options.num_ransac_hypotheses(), 2 ** 31 - 1)

    def triangulate_arrays(self, tracks: Tracks2d, track_id: Optional[ArrayLike] = None,
                           n_tracks_dev: Optional[torch.Tensor] = None, workspace_bytes: Optional[int] = None,
                           want_hypotheses: bool = False):
        """Triangulates every track of a Tracks2d (offsets, image, uv; uv float32 as DsfTracksEstimator.run_arrays
        returns it, or float64). numpy in gives numpy out; device tensors in give device tensors out with no host
        copy and no synchronisation. track_id (T,) int32 keys the sampling hash (default: the track's index);
        n_tracks_dev makes the track count a device value (see device.triangulate_tracks). With want_hypotheses the
        device result (device.TriangulationResult, with n_hyp and hyp_pair) is returned as well."""
        dev = upload.cuda_device(tracks.offsets)
        if self.options.mode == TriangulationSamplingMode.RANSAC_SAMPLE_BIASED_BASELINE:
            raise NotImplementedError("RANSAC_SAMPLE_BIASED_BASELINE is not built on the MI355X path")
        is_tensor = isinstance(tracks.offsets, torch.Tensor)
        offsets = upload.to_device(tracks.offsets, dev, torch.int32, (-1,))
        image = upload.to_device(tracks.image, dev, torch.int32, (-1,))
        uv_src = torch.as_tensor(tracks.uv)
        uv = upload.to_device(uv_src, dev, torch.float64 if uv_src.dtype == torch.float64 else torch.float32, (-1, 2))
        tid = None if track_id is None else upload.to_device(track_id, dev, torch.int32, (-1,))
        wRc, wtc, intr, valid = self._device_cameras(dev)
        res = device.triangulate_tracks(offsets, image, uv, wRc, wtc, intr, valid, MODE_TO_NATIVE[self.options.mode],
                                        self.options.reproj_error_threshold, self.options.min_triangulation_angle,
                                        self._n_hyp(), self.seed, n_tracks_dev=n_tracks_dev, track_id=tid,
                                        workspace_bytes=workspace_bytes, want_hypotheses=want_hypotheses)
        out = (res.exit_code, res.point, res.avg_err, res.inlier, res.stats)
        if is_tensor:
            out = Triangulated(*(a.to(tracks.offsets.device) for a in out))
        else:
            out = Triangulated(*(a.cpu().numpy() for a in out))
        return (out, res) if want_hypotheses else out

    def triangulate(self, track_2d: SfmTrack2d) -> Tuple[Optional[SfmTrack], Optional[float], TriangulationExitCode]:
        """The reference's triangulate(): (track with the inlier measurements and the landmark, or None; the average
        reprojection error, None for exits 1-3; the exit code)."""
        return self.triangulate_list([track_2d])[0]

    def triangulate_list(self, tracks_2d):
        """triangulate() of every track of a list, from one launch; track j's sampling hash is keyed by j."""
        n = len(tracks_2d)
        if n == 0:
            return []
        lens = [t.number_measurements() for t in tracks_2d]
        offsets = np.zeros(n + 1, np.int32)
        np.cumsum(lens, out=offsets[1:])
        image = np.array([m.i for t in tracks_2d for m in t.measurements], np.int32)
        uv = np.array([np.asarray(m.uv, np.float64).reshape(2) for t in tracks_2d for m in t.measurements],
                      np.float64).reshape(-1, 2)
        r = self.triangulate_arrays(Tracks2d(offsets, image, None, uv, None))
        out = []
        for j, track_2d in enumerate(tracks_2d):
            code = TriangulationExitCode(int(r.exit_code[j]))
            avg = None if np.isnan(r.avg_err[j]) and code.value in (1, 2, 3) else float(r.avg_err[j])
            track_3d = None
            if code == TriangulationExitCode.SUCCESS:
                track_3d = SfmTrack(r.point[j])
                for k, (i, m_uv) in enumerate(track_2d.measurements):
                    if r.inlier[offsets[j] + k]:
                        track_3d.addMeasurement(int(i), np.asarray(m_uv, np.float64))
            out.append((track_3d, avg, code))
        return out
