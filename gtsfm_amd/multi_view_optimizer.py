"""The whole back end in one device-resident call: view graph, rotation averaging, 2D tracks, translation averaging,
cameras, triangulation, the bundle-adjustment input and global bundle adjustment.

Counterpart of gtsfm/multi_view_optimizer.py:29-199 (MultiViewOptimizer, init_cameras, get_2d_tracks). The reference
wires its stages into a Dask graph; here run_arrays calls the stages' array forms one after the other on the device
tensors the batched front end leaves behind, and run keeps the reference's data signature over dicts and lists.

Out of scope, and left with the reference: create_computation_graph and Dask; every GtsfmMetricsGroup (the three
count metrics of data association are data_assoc.assemble_metrics); align_via_Sim3_to_poses of the BA input to
ground-truth poses; the debug-plot output; absolute and relative pose priors (a non-empty dict raises
NotImplementedError, as in the stages); the two-view reports, which the reference's view-graph estimator only passes
through.
"""
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from gtsfm_amd import native
from gtsfm_amd.averaging.rotation.shonan import RotationArrays
from gtsfm_amd.averaging.translation.averaging_1dsfm import TranslationArrays
from gtsfm_amd.bundle.bundle_adjustment import BaArrays, BaData
from gtsfm_amd.common import geometry, upload
from gtsfm_amd.common.sfm_track import SfmTrack
from gtsfm_amd.data_association.data_assoc import BaInputArrays
from gtsfm_amd.data_association.dsf_tracks_estimator import DsfTracksEstimator, Tracks2d, get_2d_tracks  # noqa: F401
from gtsfm_amd.data_association.point3d_initializer import DeviceCameras, Triangulated


class MultiViewArrays(NamedTuple):
    """run_arrays' result: every stage's own result object, device tensors throughout. keep (P,) uint8 is the view
    graph; cameras the tuple init_cameras_arrays returns; valid (T,) bool the tracks data association accepts; ba_input
    the masks bundle adjustment ran on; ba its result. A stage that was not reached (no pair, no rotation, no track or
    no position) and every stage after it is None."""

    keep: torch.Tensor
    rotations: Optional[RotationArrays]
    tracks: Optional[Tracks2d]
    translations: Optional[TranslationArrays]
    cameras: Optional[DeviceCameras]
    triangulated: Optional[Triangulated]
    valid: Optional[torch.Tensor]
    ba_input: Optional[BaInputArrays]
    ba: Optional[BaArrays]


def init_cameras_arrays(wRi: torch.Tensor, wti: torch.Tensor, wti_valid: torch.Tensor,
                        intrinsics: torch.Tensor) -> DeviceCameras:
    """init_cameras (multi_view_optimizer.py:171-192) on device tensors: a camera where the pose was computed. wRi
    (n_img, 3, 3) and wti (n_img, 3) float64, wti_valid (n_img,) uint8 as translation averaging returns them,
    intrinsics (n_img, 3) float64. Returns (wRc, wtc, intrinsics, cam_valid), the tuple
    DataAssociation.run_triangulation_arrays and BundleAdjustmentOptimizer.run_ba_arrays take; a camera without a pose
    holds the identity and cam_valid 0. Plain torch ops, nothing reaches the host."""
    n = wti_valid.numel()
    ok = wti_valid.reshape(n) != 0
    eye = torch.eye(3, dtype=torch.float64, device=wRi.device)
    wRc = torch.where(ok[:, None, None], wRi.reshape(n, 3, 3).to(torch.float64), eye).contiguous()
    wtc = torch.where(ok[:, None], wti.reshape(n, 3).to(torch.float64), torch.zeros_like(eye[0])).contiguous()
    return wRc, wtc, intrinsics.reshape(n, 3).to(torch.float64).contiguous(), ok.to(torch.uint8).contiguous()


class MultiViewOptimizer:
    """Averaging, data association and bundle adjustment of all images of a scene; the reference's constructor."""

    def __init__(self, rot_avg_module, trans_avg_module, data_association_module, bundle_adjustment_module,
                 view_graph_estimator=None) -> None:
        self.view_graph_estimator = view_graph_estimator
        self.rot_avg_module = rot_avg_module
        self.trans_avg_module = trans_avg_module
        self.data_association_module = data_association_module
        self.ba_optimizer = bundle_adjustment_module
        self._run_view_graph_estimator: bool = self.view_graph_estimator is not None

    def __repr__(self) -> str:
        return (f"MultiviewOptimizer: ViewGraphEstimator: {self.view_graph_estimator} RotationAveraging: "
                f"{self.rot_avg_module} TranslationAveraging: {self.trans_avg_module}")

    def run_arrays(self, pairs: torch.Tensor, i2Ri1: torch.Tensor, i2Ui1: torch.Tensor, pair_valid: torch.Tensor,
                   offsets: torch.Tensor, v_corr: torch.Tensor, kp_count: torch.Tensor, kmax: int,
                   kp_xy: torch.Tensor, intrinsics: torch.Tensor, num_images: int) -> MultiViewArrays:
        """The chain on the layout the batched front end leaves on the device: pairs (P, 2) int32, i2Ri1 (P, 3, 3) and
        i2Ui1 (P, 3) float64, pair_valid (P,) uint8 (the verifier's status and inlier-support verdict), the
        verified-correspondence CSR offsets (P + 1,) / v_corr (rows, 2) int32 of device.compact_verified, kp_count
        (n_img,) int32, kmax, kp_xy (n_img, kmax, 2) float32, intrinsics (n_img, 3) float64.

        The order is the reference's (multi_view_optimizer.py:99-155):
          1. the view graph: keep = view_graph_estimator.run_arrays(...), or pair_valid without an estimator;
          2. rotation averaging on the kept pairs. gtsfm_rotavg_shonan selects the largest connected component of the
             view graph itself, so the reference's prune_to_largest_connected_component (:123-125) is no step here: a
             camera outside that component has rot_valid 0, and every later stage ignores its edges and measurements;
          3. 2D tracks from the rows of the kept pairs (get_2d_tracks);
          4. translation averaging with edge_valid = keep, rot_valid, the track CSR and the intrinsics;
          5. init_cameras_arrays;
          6. triangulation (DataAssociation.run_triangulation_arrays);
          7. DataAssociation.assemble_arrays;
          8. run_ba_arrays with cam_valid = cam_keep, the track-valid byte = track_keep and the BA module's last
             reprojection threshold, as run_ba does. The BA module is used as it was given: one built with
             refine_calibration=True refines the calibration, and its BaArrays.calib is part of the result (`run`
             builds the optimised and filtered cameras from it); the dense stage does not read it yet.

        Host synchronisations are those of the stages and no other: the track counts that size the track arrays
        (DsfTracksEstimator.run_arrays); translation averaging's `counts` and its recovery's control scalars; the
        rotation staircase's control scalars; bundle adjustment's control scalars. The status and camera count of the
        two averaging stages are read from their stats after those calls have synchronised; they decide whether the
        chain stops early. Nothing else is copied to the host: the cameras, the triangulation, its valid mask and
        the assembled masks go from stage to stage as device tensors."""
        native.require_gpu()
        dev = pairs.device
        pairs = pairs.to(torch.int32).reshape(-1, 2).contiguous()
        P = pairs.shape[0]
        keep = (pair_valid.reshape(P) != 0).to(torch.uint8).contiguous()
        nothing = MultiViewArrays(keep, None, None, None, None, None, None, None, None)
        if P == 0 or num_images <= 0:
            return nothing
        i2Ri1 = i2Ri1.reshape(P, 3, 3).contiguous()
        i2Ui1 = i2Ui1.reshape(P, 3).contiguous()
        if self._run_view_graph_estimator:
            kept, _, _ = self.view_graph_estimator.run_arrays(pairs, i2Ri1, valid=keep, num_images=num_images)
            keep = (kept.to(dev) != 0).to(torch.uint8).contiguous()
        rot = self.rot_avg_module.run_rotation_averaging_arrays(pairs, i2Ri1, keep, num_images)
        out = MultiViewArrays(keep, rot, None, None, None, None, None, None, None)
        rot_stats = rot.stats.cpu().numpy()
        if int(rot_stats[11]) in (native.RA_STATUS_NOTHING, native.RA_STATUS_NOT_FINITE) or rot_stats[9] == 0:
            return out
        tracks = DsfTracksEstimator().run_arrays(pairs, offsets, v_corr, kp_count, kmax, valid=keep, kp_xy=kp_xy)
        out = out._replace(tracks=tracks)
        if tracks.offsets.numel() < 2:  # no track: no camera edge, an empty scene (gtsfm_data.py:265-266)
            return out
        trans = self.trans_avg_module.run_translation_averaging_arrays(
            pairs, i2Ui1, rot.wRi, edge_valid=keep, rot_valid=rot.rot_valid, track_offsets=tracks.offsets,
            track_img=tracks.image, track_uv=tracks.uv, intrinsics=intrinsics)
        out = out._replace(translations=trans)
        trans_stats = trans.stats.cpu().numpy()
        if int(trans_stats[9]) != native.TA_STATUS_OK or trans_stats[8] == 0:
            return out
        cams = init_cameras_arrays(rot.wRi, trans.wti, trans.wti_valid, intrinsics)
        tri, valid = self.data_association_module.run_triangulation_arrays(cams, tracks)
        ba_in = self.data_association_module.assemble_arrays(tracks, tri, valid, cams[3])
        ba = self.ba_optimizer.run_ba_arrays((cams[0], cams[1], cams[2], ba_in.cam_keep), tracks, tri,
                                             ba_in.track_keep,
                                             reproj_error_thresh=self.ba_optimizer._reproj_error_thresholds[-1])
        return out._replace(cameras=cams, triangulated=tri, valid=valid, ba_input=ba_in, ba=ba)

    def run(self, num_images: int, keypoints_list: List[object], i2Ri1_dict: Dict[Tuple[int, int], Optional[object]],
            i2Ui1_dict: Dict[Tuple[int, int], Optional[object]], v_corr_idxs_dict: Dict[Tuple[int, int], np.ndarray],
            all_intrinsics: List[Optional[object]], relative_pose_priors: Optional[dict] = None,
            ) -> Tuple[BaData, BaData, BaData]:
        """The reference's data signature without Dask. keypoints_list holds the Keypoints of every image (None = no
        detections); i2Ri1_dict / i2Ui1_dict values are Rot3 / Unit3, arrays or None; v_corr_idxs_dict maps (i1, i2)
        to (K, 2) keypoint index rows; all_intrinsics holds Cal3Bundler or None. Returns (ba_input, ba_output,
        ba_filtered): the cameras and 3D tracks bundle adjustment started from, the optimised ones, and those that
        pass its reprojection filter. Empty inputs, a stage that yields no camera and an empty assembled component
        give three empty BaData. Raises RuntimeError when rotation averaging ends without its certificate, as
        ShonanRotationAveraging.run_rotation_averaging does."""
        if relative_pose_priors:
            raise NotImplementedError("relative-pose priors are not built into the MI355X back end; pass an empty "
                                      "relative_pose_priors")
        empty = (BaData({}, []), BaData({}, []), BaData({}, []))
        pair_keys = list(i2Ri1_dict.keys())
        if num_images <= 0 or not pair_keys:
            return empty
        P = len(pair_keys)
        R = np.tile(np.eye(3), (P, 1, 1))
        U = np.zeros((P, 3))
        ok = np.zeros(P, np.uint8)
        rows = []
        for k, key in enumerate(pair_keys):
            r, u = i2Ri1_dict[key], i2Ui1_dict.get(key)
            if r is not None and u is not None:
                R[k] = geometry.rotation_matrix(r)
                U[k] = geometry.unit_vector(u) if hasattr(u, "point3") else np.asarray(u, np.float64).reshape(3)
                ok[k] = 1
            corr = v_corr_idxs_dict.get(key)
            rows.append(np.zeros((0, 2), np.int32) if corr is None else np.asarray(corr).reshape(-1, 2).astype(np.int32))
        if not ok.any():
            return empty
        offsets = np.zeros(P + 1, np.int32)
        np.cumsum([len(r) for r in rows], out=offsets[1:])
        v_corr = np.concatenate(rows).reshape(-1, 2)
        coords = [None if kps is None else np.asarray(kps.coordinates).reshape(-1, 2) for kps in keypoints_list]
        kp_count = np.array([0 if c is None else len(c) for c in coords], np.int32)
        kmax = max(int(kp_count.max()), 1)
        kp_xy = np.zeros((num_images, kmax, 2), np.float32)
        for i, c in enumerate(coords):
            if c is not None:
                kp_xy[i, : len(c)] = c
        intr = np.tile(np.array([1.0, 0.0, 0.0]), (num_images, 1))
        for i, cal in enumerate(all_intrinsics):
            if cal is not None:
                intr[i] = geometry.calibration_params(cal)
        dev = upload.cuda_device()
        r = self.run_arrays(*(upload.to_device(a, dev) for a in (np.asarray(pair_keys, np.int32).reshape(-1, 2), R, U,
                                                                   ok, offsets, v_corr, kp_count)),
                            kmax, upload.to_device(kp_xy, dev), upload.to_device(intr, dev), num_images)
        if r.rotations is not None and int(r.rotations.stats[11].item()) == native.RA_STATUS_UNCERTIFIED:
            raise RuntimeError("Shonan rotation averaging reached p_max without an optimality certificate")
        if r.ba is None:
            return empty
        t_off, t_img, t_kp = (a.cpu().numpy() for a in (r.tracks.offsets, r.tracks.image, r.tracks.keypoint))
        inlier = r.triangulated.inlier.cpu().numpy()

        def data(wRc, wtc, point, cam_mask, track_mask, calib=None) -> BaData:
            """calib: the (n_img, 5) calibration a BA module with refine_calibration=True returns, or None."""
            wRc, wtc, point = wRc.cpu().numpy(), wtc.cpu().numpy(), point.cpu().numpy()
            calib = None if calib is None else calib.cpu().numpy()
            cams = {int(i): geometry.PinholeCameraCal3Bundler(
                        geometry.Pose3(geometry.Rot3(wRc[i]), wtc[i]),
                        all_intrinsics[i] if calib is None else geometry.Cal3Bundler(*(float(v) for v in calib[i])))
                    for i in np.flatnonzero(cam_mask.cpu().numpy())}
            cals = None if calib is None else {i: calib[i].copy() for i in cams}
            tracks = []
            for t in np.flatnonzero(track_mask.cpu().numpy()):
                track = SfmTrack(point[t])
                for m in range(t_off[t], t_off[t + 1]):
                    if inlier[m]:
                        track.addMeasurement(int(t_img[m]),
                                             np.asarray(coords[t_img[m]][t_kp[m]], np.float64).reshape(2))
                tracks.append(track)
            return BaData(cams, tracks, cals)

        cam0 = r.cameras
        ba_input = data(cam0[0], cam0[1], r.triangulated.point, r.ba_input.cam_keep, r.ba_input.track_keep)
        if not ba_input.cameras:
            return empty
        if int(r.ba.stats[9].item()) == native.GBA_STATUS_NOTHING:  # bundle_adjustment.py:319-324
            return ba_input, ba_input, ba_input
        ba_output = data(r.ba.wRc, r.ba.wtc, r.ba.point, r.ba_input.cam_keep, r.ba_input.track_keep, r.ba.calib)
        ba_filtered = data(r.ba.wRc, r.ba.wtc, r.ba.point, r.ba.cam_keep, r.ba.track_keep, r.ba.calib)
        return ba_input, ba_output, ba_filtered
