"""Bundle adjustment of all cameras and landmarks on the MI355X.

Drop-in for gtsfm/bundle/bundle_adjustment.py:58-397 (BundleAdjustmentOptimizer): the reference builds a GTSAM factor
graph (reprojection factors, a pose prior on the first camera, a point prior on the first landmark) and runs one
LevenbergMarquardtOptimizer; here that is one gtsfm_global_ba call (libgtsfm_hip.so; semantics, the solver and the
stated approximations in include/gtsfm_hip.h). With refine_calibration=False (the default) calibration is held fixed,
the limit of the reference's 1e-5 calibration prior: shared_calib and calibration_prior_noise_sigma do not enter that
call, and non-zero k1 / k2 is refused by geometry.calibration_params. With refine_calibration=True the call is
gtsfm_global_ba_calib: the Cal3Bundler (f, k1, k2) of every modelled camera, or of one camera shared by all when
shared_calib=True, is a variable under a prior of calibration_prior_noise_sigma (bundle_adjustment.py:103-131,
:180-208), distorted cameras are accepted and the results carry the refined calibration. Relative-pose priors
(BetweenFactorPose3) are not built: a non-empty dict raises NotImplementedError. evaluate(), the metrics and
create_computation_graph (Dask) stay with the reference.

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


ALL_STAGES = "all-stages"  # run_ba_arrays' default threshold: every stage of the constructor's list (see there)


class BaData(NamedTuple):
    """The part of the reference's GtsfmData that bundle adjustment reads and writes: cameras {image index: camera}
    and the 3D tracks. calibrations, set on results of refine_calibration=True, is {image index: (f, k1, k2, u0, v0)},
    the refined rows the cameras' Cal3Bundlers were built from."""

    cameras: Dict[int, object]
    tracks: List[SfmTrack]
    calibrations: Optional[Dict[int, np.ndarray]] = None

    def number_tracks(self) -> int:
        return len(self.tracks)

    def get_valid_camera_indices(self) -> List[int]:
        return sorted(i for i, c in self.cameras.items() if c is not None)


class BaArrays(NamedTuple):
    """run_ba_arrays' result, device tensors: optimised wRc (n_img, 3, 3), wtc (n_img, 3) and point (T, 3); track_keep
    (T,) and cam_keep (n_img,) uint8 (the tracks and cameras of the reference's filtered_result); stats (10,) float64
    in the order of native.GBA_STATS_FIELDS. With refine_calibration=True: calib (n_img, 5) = (f, k1, k2, u0, v0), refined
    for the modelled cameras, and stats (12,) in the order of native.GBA_CALIB_STATS_FIELDS."""

    wRc: torch.Tensor
    wtc: torch.Tensor
    point: torch.Tensor
    track_keep: torch.Tensor
    cam_keep: torch.Tensor
    stats: torch.Tensor
    calib: Optional[torch.Tensor] = None


def camera_arrays5(cameras: Dict[int, object]):
    """camera_arrays with the full Cal3Bundler row: (wRc, wtc, calib (n_img, 5) = (f, k1, k2, u0, v0), valid)."""
    n = max(int(i) for i in cameras) + 1
    wRc, wtc = np.tile(np.eye(3), (n, 1, 1)), np.zeros((n, 3))
    calib = np.tile(np.array([1.0, 0.0, 0.0, 0.0, 0.0]), (n, 1))
    valid = np.zeros(n, np.uint8)
    for i, cam in cameras.items():
        if cam is None or not 0 <= int(i) < n:
            continue
        wRc[i], wtc[i] = geometry.camera_pose(cam)
        calib[i] = geometry.calibration_params5(cam.calibration())
        valid[i] = 1
    return wRc, wtc, calib, valid


class BundleAdjustmentOptimizer:
    """Refines camera poses and landmarks together and, with refine_calibration=True, the cameras' calibration; the
    reference's constructor arguments plus the PCG controls and that switch. shared_calib and
    calibration_prior_noise_sigma act only with refine_calibration=True."""

    def __init__(self, reproj_error_thresholds: List[Optional[float]] = [None], robust_measurement_noise: bool = False,
                 shared_calib: bool = False, max_iterations: Optional[int] = None,
                 cam_pose3_prior_noise_sigma: float = 0.1, calibration_prior_noise_sigma: float = 1e-5,
                 measurement_noise_sigma: float = 1.0, pcg_rel_tol: float = 1e-10, pcg_max_iter: int = 2000,
                 refine_calibration: bool = False) -> None:
        self._refine_calibration = refine_calibration
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

    def _solver_options(self, reproj_error_thresh: Optional[float]) -> dict:
        """The keyword arguments device.global_ba and device.global_ba_calib share."""
        return dict(robust=self._robust_measurement_noise, measurement_sigma=self._measurement_noise_sigma,
                    cam_pose3_prior_sigma=self._cam_pose3_prior_noise_sigma, max_iterations=self._max_iterations or 0,
                    pcg_rel_tol=self._pcg_rel_tol, pcg_max_iter=self._pcg_max_iter,
                    reproj_error_thresh=float("inf") if reproj_error_thresh is None else float(reproj_error_thresh))

    def _calib_options(self) -> dict:
        return dict(shared_calib=self._shared_calib, calibration_prior_sigma=self._calibration_prior_noise_sigma)

    def run_ba_arrays(self, cameras: Dict[int, object], tracks: Tracks2d, triangulated: Triangulated,
                      valid: Optional[torch.Tensor], reproj_error_thresh: Optional[float] = ALL_STAGES,
                      n_tracks_dev: Optional[torch.Tensor] = None,
                      relative_pose_priors: Optional[dict] = None) -> BaArrays:
        """One bundle adjustment straight from the device tensors of DsfTracksEstimator.run_arrays (tracks) and
        DataAssociation.run_triangulation_arrays (triangulated, valid): landmarks triangulated.point, factors the
        inlier measurements (triangulated.inlier) of the valid tracks. cameras is {image index: camera or None}, or a
        tuple of device tensors (wRc, wtc, intrinsics, cam_valid). Nothing is copied to the host beyond the solver's
        control scalars.

        reproj_error_thresh: a threshold, or None for no filter. Left at its default it is None with
        refine_calibration=False; with refine_calibration=True it stands for every stage of the constructor's
        reproj_error_thresholds: one optimisation per threshold, each from the same initial poses and landmarks (the
        reference's run_ba hands the same initial_data to every stage, :381-389) and from the calibration the stage
        before refined, which is also where its calibration prior sits; the last stage is returned. With
        refine_calibration=True the intrinsics of a camera tuple may be (n_img, 5) = (f, k1, k2, u0, v0)."""
        native.require_gpu()
        self._check_priors(relative_pose_priors)
        dev = tracks.offsets.device
        if self._refine_calibration:
            return self._run_ba_arrays_calib(cameras, tracks, triangulated, valid, reproj_error_thresh, n_tracks_dev)
        if reproj_error_thresh is ALL_STAGES:
            reproj_error_thresh = None
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
            wRc.contiguous(), wtc.contiguous(), intr.contiguous(), cam_valid,
            **self._solver_options(reproj_error_thresh), n_tracks=T, n_tracks_dev=n_tracks_dev)
        return BaArrays(r.wRc, r.wtc, r.point, r.track_keep, r.cam_keep, r.stats)

    def _run_ba_arrays_calib(self, cameras, tracks: Tracks2d, triangulated: Triangulated,
                             valid: Optional[torch.Tensor], reproj_error_thresh, n_tracks_dev) -> BaArrays:
        """run_ba_arrays with refine_calibration=True: gtsfm_global_ba_calib, once per stage."""
        dev = tracks.offsets.device
        if isinstance(cameras, dict):
            wRc, wtc, calib, cam_valid = (upload.to_device(a, dev) for a in camera_arrays5(cameras))
        else:
            wRc, wtc, calib, cam_valid = tuple(cameras)
            if calib.shape[-1] == 3:  # (f, u0, v0): no distortion
                zero = torch.zeros_like(calib[:, :1])
                calib = torch.cat([calib[:, :1], zero, zero, calib[:, 1:]], dim=1)
        stages = list(self._reproj_error_thresholds) if reproj_error_thresh is ALL_STAGES else [reproj_error_thresh]
        T = triangulated.exit_code.numel()
        uv = tracks.uv if tracks.uv.dtype in (torch.float32, torch.float64) else tracks.uv.to(torch.float32)
        csr = (tracks.offsets.to(torch.int32).contiguous(), tracks.image.to(torch.int32).contiguous(),
               uv.reshape(-1, 2).contiguous(), triangulated.point.contiguous(),
               None if valid is None else valid.to(torch.uint8).contiguous(), triangulated.inlier.contiguous())
        for thresh in stages:
            r = device.global_ba_calib(*csr, wRc.contiguous(), wtc.contiguous(), calib.contiguous(), cam_valid,
                                       **self._solver_options(thresh), **self._calib_options(), n_tracks=T,
                                       n_tracks_dev=n_tracks_dev)
            calib = r.calib
        return BaArrays(r.wRc, r.wtc, r.point, r.track_keep, r.cam_keep, r.stats, r.calib)

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
        refine = self._refine_calibration
        cams5 = camera_arrays5(initial_data.cameras) if refine else None
        cams = None if refine else camera_arrays(initial_data.cameras)
        lens = [t.numberMeasurements() for t in initial_data.tracks]
        offsets = np.zeros(n + 1, np.int32)
        np.cumsum(lens, out=offsets[1:])
        meas = [t.measurement(k) for t in initial_data.tracks for k in range(t.numberMeasurements())]
        image = np.array([m[0] for m in meas], np.int32)
        uv = np.array([np.asarray(m[1], np.float64).reshape(2) for m in meas], np.float64).reshape(-1, 2)
        point = np.array([np.asarray(t.point3(), np.float64).reshape(3) for t in initial_data.tracks]).reshape(-1, 3)
        csr = (upload.to_device(a, dev) for a in (offsets, image, uv, point))
        if refine:
            r = device.global_ba_calib(*csr, None, None, *(upload.to_device(a, dev) for a in cams5),
                                       **self._solver_options(reproj_error_thresh), **self._calib_options())
            calib = r.calib.cpu().numpy()
        else:
            r = device.global_ba(
                *csr, None, None,
                *(upload.to_device(a, dev) for a in (cams.wRc, cams.wtc, cams.intrinsics, cams.valid)),
                **self._solver_options(reproj_error_thresh))
        wRc, wtc, pts = r.wRc.cpu().numpy(), r.wtc.cpu().numpy(), r.point.cpu().numpy()
        keep, cam_keep, stats = r.track_keep.cpu().numpy(), r.cam_keep.cpu().numpy(), r.stats.cpu().numpy()
        if int(stats[9]) == native.GBA_STATUS_NOTHING:
            return initial_data, initial_data, [False] * n, 0.0
        opt_cams = {}
        for i, cam in initial_data.cameras.items():
            if cam is None:
                opt_cams[i] = None
                continue
            cal = geometry.Cal3Bundler(*(float(v) for v in calib[i])) if refine else cam.calibration()
            opt_cams[i] = geometry.PinholeCameraCal3Bundler(geometry.Pose3(geometry.Rot3(wRc[i]), wtc[i]), cal)
        opt_tracks = []
        for j, t in enumerate(initial_data.tracks):
            nt = SfmTrack(pts[j])
            for k in range(t.numberMeasurements()):
                i, m_uv = t.measurement(k)
                nt.addMeasurement(int(i), np.asarray(m_uv, np.float64))
            opt_tracks.append(nt)
        cals = {i: calib[i].copy() for i, c in opt_cams.items() if c is not None} if refine else None
        optimized = BaData(opt_cams, opt_tracks, cals)
        if reproj_error_thresh is None:  # bundle_adjustment.py:353-355: no filter at all
            return optimized, optimized, [True] * n, float(stats[1])
        filtered = BaData({i: c for i, c in opt_cams.items() if c is not None and cam_keep[i]},
                          [t for j, t in enumerate(opt_tracks) if keep[j]],
                          None if cals is None else {i: k for i, k in cals.items() if cam_keep[i]})
        return optimized, filtered, [bool(k) for k in keep], float(stats[1])

    def run_ba(self, initial_data: BaData, absolute_pose_priors: List[Optional[object]],
               relative_pose_priors: Dict[Tuple[int, int], object], verbose: bool = True,
               ) -> Tuple[BaData, BaData, List[bool]]:
        """The reference's run_ba (bundle_adjustment.py:359-397) as written: its loop hands the same initial_data to
        every stage (:381-389), so what it returns is the result of the LAST threshold alone. The optimisation does not
        depend on the threshold, so it is run once and the last threshold's filter applied.

        With refine_calibration=True every stage is run: each starts from the initial poses and landmarks, as in the
        reference, and from the calibration the stage before refined; the last stage is returned."""
        if self._refine_calibration:
            data = initial_data
            for thresh in self._reproj_error_thresholds:
                optimized, filtered, mask, _ = self.run_ba_stage_with_filtering(
                    data, absolute_pose_priors, relative_pose_priors, thresh, verbose)
                data = BaData({i: None if c is None or optimized.cameras.get(i) is None else
                               geometry.PinholeCameraCal3Bundler(c.pose(), optimized.cameras[i].calibration())
                               for i, c in initial_data.cameras.items()}, initial_data.tracks)
            return optimized, filtered, mask
        optimized, filtered, mask, _ = self.run_ba_stage_with_filtering(
            initial_data, absolute_pose_priors, relative_pose_priors, self._reproj_error_thresholds[-1], verbose)
        return optimized, filtered, mask
