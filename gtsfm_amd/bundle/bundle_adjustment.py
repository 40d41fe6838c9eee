"""Bundle adjustment of all cameras and landmarks on the MI355X.

Drop-in for gtsfm/bundle/bundle_adjustment.py:58-397 (BundleAdjustmentOptimizer): the reference builds a GTSAM factor
graph (reprojection factors, a pose prior on the first camera, a point prior on the first landmark) and runs one
LevenbergMarquardtOptimizer; here that is one gtsfm_global_ba call (libgtsfm_hip.so; semantics, the solver and the
stated approximations in include/gtsfm_hip.h). Calibration is held fixed, so shared_calib and
calibration_prior_noise_sigma are accepted and have no effect; non-zero k1 / k2 is refused by
geometry.calibration_params. Relative-pose priors (BetweenFactorPose3) are not built: a non-empty dict raises
NotImplementedError. evaluate(), the metrics and create_computation_graph (Dask) stay with the reference.

Two forms, as in data_association/data_assoc.py: run_ba_arrays takes and returns device tensors (only the solver's
control scalars reach the host); run_ba_stage_with_filtering / run_ba keep the reference's signatures over a BaData
(a camera dict and a list of SfmTrack) in place of GtsfmData.
"""
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from gtsfm_amd import device, native
from gtsfm_amd.common import geometry, upload
from gtsfm_amd.common.sfm_track import SfmTrack
from gtsfm_amd.data_association.dsf_tracks_estimator import Tracks2d
from gtsfm_amd.data_association.point3d_initializer import Triangulated, camera_arrays


class BaData(NamedTuple):
    """The part of the reference's GtsfmData that bundle adjustment reads and writes: cameras {image index: camera}
    and the 3D tracks."""

    cameras: Dict[int, object]
    tracks: List[SfmTrack]

    def number_tracks(self) -> int:
        return len(self.tracks)

    def get_valid_camera_indices(self) -> List[int]:
        return sorted(i for i, c in self.cameras.items() if c is not None)


class BaArrays(NamedTuple):
    """run_ba_arrays' result, device tensors: optimised wRc (n_img, 3, 3), wtc (n_img, 3) and point (T, 3); track_keep
    (T,) and cam_keep (n_img,) uint8 (the tracks and cameras of the reference's filtered_result); stats (10,) float64
    in the order of native.GBA_STATS_FIELDS."""

    wRc: torch.Tensor
    wtc: torch.Tensor
    point: torch.Tensor
    track_keep: torch.Tensor
    cam_keep: torch.Tensor
    stats: torch.Tensor


class BundleAdjustmentOptimizer:
    """Refines camera poses and landmarks together; the reference's constructor arguments plus the PCG controls."""

    def __init__(self, reproj_error_thresholds: List[Optional[float]] = [None], robust_measurement_noise: bool = False,
                 shared_calib: bool = False, max_iterations: Optional[int] = None,
                 cam_pose3_prior_noise_sigma: float = 0.1, calibration_prior_noise_sigma: float = 1e-5,
                 measurement_noise_sigma: float = 1.0, pcg_rel_tol: float = 1e-10, pcg_max_iter: int = 2000) -> None:
        self._reproj_error_thresholds = reproj_error_thresholds
        self._robust_measurement_noise = robust_measurement_noise
        self._shared_calib = shared_calib
        self._max_iterations = max_iterations
        self._cam_pose3_prior_noise_sigma = cam_pose3_prior_noise_sigma
        self._calibration_prior_noise_sigma = calibration_prior_noise_sigma
        self._measurement_noise_sigma = measurement_noise_sigma
        self._pcg_rel_tol = pcg_rel_tol
        self._pcg_max_iter = pcg_max_iter

    @staticmethod
    def _check_priors(relative_pose_priors) -> None:
        if relative_pose_priors:
            raise NotImplementedError("relative-pose priors (BetweenFactorPose3) are not built into gtsfm_global_ba; "
                                      "pass an empty relative_pose_priors")

    def run_ba_arrays(self, cameras: Dict[int, object], tracks: Tracks2d, triangulated: Triangulated,
                      valid: Optional[torch.Tensor], reproj_error_thresh: Optional[float] = None,
                      n_tracks_dev: Optional[torch.Tensor] = None,
                      relative_pose_priors: Optional[dict] = None) -> BaArrays:
        """One bundle adjustment straight from the device tensors of DsfTracksEstimator.run_arrays (tracks) and
        DataAssociation.run_triangulation_arrays (triangulated, valid): landmarks triangulated.point, factors the
        inlier measurements (triangulated.inlier) of the valid tracks. cameras is {image index: camera or None}, or a
        tuple of device tensors (wRc, wtc, intrinsics, cam_valid). Nothing is copied to the host beyond the solver's
        control scalars."""
        native.require_gpu()
        self._check_priors(relative_pose_priors)
        dev = tracks.offsets.device
        if isinstance(cameras, dict):
            c = camera_arrays(cameras)
            cams = tuple(upload.to_device(a, dev) for a in (c.wRc, c.wtc, c.intrinsics, c.valid))
        else:
            cams = tuple(cameras)
        wRc, wtc, intr, cam_valid = cams
        T = triangulated.exit_code.numel()
        uv = tracks.uv if tracks.uv.dtype in (torch.float32, torch.float64) else tracks.uv.to(torch.float32)
        r = device.global_ba(
            tracks.offsets.to(torch.int32).contiguous(), tracks.image.to(torch.int32).contiguous(),
            uv.reshape(-1, 2).contiguous(), triangulated.point.contiguous(),
            None if valid is None else valid.to(torch.uint8).contiguous(), triangulated.inlier.contiguous(),
            wRc.contiguous(), wtc.contiguous(), intr.contiguous(), cam_valid, robust=self._robust_measurement_noise,
            measurement_sigma=self._measurement_noise_sigma, cam_pose3_prior_sigma=self._cam_pose3_prior_noise_sigma,
            max_iterations=self._max_iterations or 0, pcg_rel_tol=self._pcg_rel_tol, pcg_max_iter=self._pcg_max_iter,
            reproj_error_thresh=float("inf") if reproj_error_thresh is None else float(reproj_error_thresh),
            n_tracks=T, n_tracks_dev=n_tracks_dev)
        return BaArrays(r.wRc, r.wtc, r.point, r.track_keep, r.cam_keep, r.stats)

    def run_ba_stage_with_filtering(self, initial_data: BaData, absolute_pose_priors: List[Optional[object]],
                                    relative_pose_priors: Dict[Tuple[int, int], object],
                                    reproj_error_thresh: Optional[float], verbose: bool = True,
                                    ) -> Tuple[BaData, BaData, List[bool], float]:
        """(optimised data, filtered data, valid mask over the input tracks, final error), as the reference's
        run_ba_stage_with_filtering (bundle_adjustment.py:292-357). The filtered data holds the kept tracks and the
        cameras that still see one of them. absolute_pose_priors is unused, as in the reference (:165-166)."""
        self._check_priors(relative_pose_priors)
        n = initial_data.number_tracks()
        if n == 0 or len(initial_data.get_valid_camera_indices()) == 0:
            return initial_data, initial_data, [False] * n, 0.0
        dev = upload.cuda_device()
        cams = camera_arrays(initial_data.cameras)
        lens = [t.numberMeasurements() for t in initial_data.tracks]
        offsets = np.zeros(n + 1, np.int32)
        np.cumsum(lens, out=offsets[1:])
        meas = [t.measurement(k) for t in initial_data.tracks for k in range(t.numberMeasurements())]
        image = np.array([m[0] for m in meas], np.int32)
        uv = np.array([np.asarray(m[1], np.float64).reshape(2) for m in meas], np.float64).reshape(-1, 2)
        point = np.array([np.asarray(t.point3(), np.float64).reshape(3) for t in initial_data.tracks]).reshape(-1, 3)
        csr = (upload.to_device(a, dev) for a in (offsets, image, uv, point))
        r = device.global_ba(
            *csr, None, None, *(upload.to_device(a, dev) for a in (cams.wRc, cams.wtc, cams.intrinsics, cams.valid)),
            robust=self._robust_measurement_noise,
            measurement_sigma=self._measurement_noise_sigma, cam_pose3_prior_sigma=self._cam_pose3_prior_noise_sigma,
            max_iterations=self._max_iterations or 0, pcg_rel_tol=self._pcg_rel_tol, pcg_max_iter=self._pcg_max_iter,
            reproj_error_thresh=float("inf") if reproj_error_thresh is None else float(reproj_error_thresh))
        wRc, wtc, pts = r.wRc.cpu().numpy(), r.wtc.cpu().numpy(), r.point.cpu().numpy()
        keep, cam_keep, stats = r.track_keep.cpu().numpy(), r.cam_keep.cpu().numpy(), r.stats.cpu().numpy()
        if int(stats[9]) == native.GBA_STATUS_NOTHING:
            return initial_data, initial_data, [False] * n, 0.0
        opt_cams = {}
        for i, cam in initial_data.cameras.items():
            if cam is None:
                opt_cams[i] = None
                continue
            opt_cams[i] = geometry.PinholeCameraCal3Bundler(geometry.Pose3(geometry.Rot3(wRc[i]), wtc[i]),
                                                            cam.calibration())
        opt_tracks = []
        for j, t in enumerate(initial_data.tracks):
            nt = SfmTrack(pts[j])
            for k in range(t.numberMeasurements()):
                i, m_uv = t.measurement(k)
                nt.addMeasurement(int(i), np.asarray(m_uv, np.float64))
            opt_tracks.append(nt)
        optimized = BaData(opt_cams, opt_tracks)
        if reproj_error_thresh is None:  # bundle_adjustment.py:353-355: no filter at all
            return optimized, optimized, [True] * n, float(stats[1])
        filtered = BaData({i: c for i, c in opt_cams.items() if c is not None and cam_keep[i]},
                          [t for j, t in enumerate(opt_tracks) if keep[j]])
        return optimized, filtered, [bool(k) for k in keep], float(stats[1])

    def run_ba(self, initial_data: BaData, absolute_pose_priors: List[Optional[object]],
               relative_pose_priors: Dict[Tuple[int, int], object], verbose: bool = True,
               ) -> Tuple[BaData, BaData, List[bool]]:
        """The reference's run_ba (bundle_adjustment.py:359-397) as written: its loop hands the same initial_data to
        every stage (:381-389), so what it returns is the result of the LAST threshold alone. The optimisation does not
        depend on the threshold, so it is run once and the last threshold's filter applied."""
        optimized, filtered, mask, _ = self.run_ba_stage_with_filtering(
            initial_data, absolute_pose_priors, relative_pose_priors, self._reproj_error_thresholds[-1], verbose)
        return optimized, filtered, mask
