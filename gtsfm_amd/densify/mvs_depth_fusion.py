"""Dense multi-view stereo around a pluggable depth estimator, device-resident: source views and depth ranges from the
bundle-adjusted tracks, the estimator's depth and confidence maps filtered and fused into a coloured point cloud.

Counterpart of gtsfm/densify/mvs_patchmatchnet.py:49-437 (MVSPatchmatchNet.densify, filter_depth,
compute_filtered_reprojection_error) and gtsfm/densify/patchmatchnet_data.py:28-162 without the network: the depth
estimator is any callable `depth_estimator(images, proj_inputs, depth_range) -> (depth, confidence)` over device
tensors, where images is (n_valid, H, W, 3) uint8 in pm_i order, proj_inputs the tuple (wRc (n_valid, 3, 3), wtc
(n_valid, 3), intrinsics (n_valid, 3), src_views (n_valid, S) int32) and depth_range (n_valid, 2); it returns two
(n_valid, H, W) float32 tensors. gtsfm_amd.densify.patchmatchnet.PatchmatchNetDepthEstimator is that callable on the HIP
PatchmatchNet, and gtsfm_amd.densify.mvs_patchmatchnet.MVSPatchmatchNet the two together.

Not built: the reference's resize of every image to the size of image 0 (all images must share one size: ValueError),
the quantiles of the reprojection errors (count, mean, min and max are reported), .ply output, Dask.
"""
from typing import Callable, Dict, NamedTuple, Optional, Tuple

import numpy as np
import torch

from gtsfm_amd import device, native
from gtsfm_amd.common import geometry, upload
from gtsfm_amd.densify.mvs_base import MVSBase

MAX_GEOMETRIC_PIXEL_THRESH = 1.0      # mvs_patchmatchnet.py's defaults
MAX_GEOMETRIC_DEPTH_THRESH = 0.01
MIN_CONFIDENCE_THRESH = 0.8
MIN_NUM_CONSISTENT_VIEWS = 1
NUM_VIEWS = 5


class MvsViews(NamedTuple):
    """select_views_arrays' result on the device, sliced to the valid cameras: img_to_pm (n_img,) int32 (-1 = not
    valid), pm_to_img (n_valid,) int32, scores (n_valid, n_valid) float64, scores_fixed the same as int64 in units of
    2^-40 (byte-identical from launch to launch), src_views (n_valid, V - 1) int32, depth_range (n_valid, 2) float64,
    stats (4,) int64 (native.MVS_VIEWS_STATS_FIELDS)."""

    img_to_pm: torch.Tensor
    pm_to_img: torch.Tensor
    scores: torch.Tensor
    scores_fixed: torch.Tensor
    src_views: torch.Tensor
    depth_range: torch.Tensor
    stats: torch.Tensor


class DensePoints(NamedTuple):
    """fuse_depth_arrays' result on the device: points (N, 3) float64 and colors (N, 3) uint8 in canonical order
    (views ascending, then row-major), view_offset (n_valid + 1,) int64, fused (n_valid, H, W) float32, mask (n_valid,
    H, W) uint8, counts (n_valid, 4) int64 (native.MVS_FUSE_COUNT_FIELDS), err (n_valid, 3) float64."""

    points: torch.Tensor
    colors: torch.Tensor
    view_offset: torch.Tensor
    fused: torch.Tensor
    mask: torch.Tensor
    counts: torch.Tensor
    err: torch.Tensor


def select_views_arrays(cameras, tracks, point: torch.Tensor, track_keep: Optional[torch.Tensor],
                        inlier: Optional[torch.Tensor], max_num_views: int = NUM_VIEWS) -> MvsViews:
    """select_src_views_depth_ranges on device tensors. cameras = (wRc, wtc, intrinsics, cam_keep) as bundle
    adjustment returns them, tracks the Tracks2d CSR (offsets, image), point (T, 3) float64, track_keep (T,) and inlier
    (n_meas,) uint8 or None. One host synchronisation: the number of valid cameras is read to slice the outputs."""
    wRc, wtc, _, cam_keep = cameras
    track_keep, inlier, cam_keep = (None if m is None else (m != 0).to(torch.uint8).contiguous()
                                    for m in (track_keep, inlier, cam_keep))
    r = device.mvs_select_views(tracks.offsets, tracks.image, point.contiguous(), track_keep, inlier,
                                wRc.contiguous(), wtc.contiguous(), cam_keep, max_num_views)
    nv, picks = (int(v) for v in r.stats[:2].tolist())
    fixed = r.scores[:nv, :nv].contiguous()
    return MvsViews(r.img_to_pm, r.pm_to_img[:nv].contiguous(), fixed.to(torch.float64) / native.MVS_SCORE_SCALE,
                    fixed, r.src_views[:nv, :picks].contiguous(), r.depth_range[:nv].contiguous(), r.stats)


def valid_cameras(cameras, views: MvsViews) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(wRc, wtc, intrinsics) of the valid cameras in pm_i order."""
    idx = views.pm_to_img.long()
    n = cameras[1].numel() // 3
    return (cameras[0].reshape(n, 3, 3)[idx].contiguous(), cameras[1].reshape(n, 3)[idx].contiguous(),
            cameras[2].reshape(n, 3)[idx].contiguous())


def fuse_depth_arrays(depth: torch.Tensor, confidence: torch.Tensor, images_u8: torch.Tensor, cameras,
                      views: MvsViews, max_geo_pixel_thresh: float = MAX_GEOMETRIC_PIXEL_THRESH,
                      max_geo_depth_thresh: float = MAX_GEOMETRIC_DEPTH_THRESH,
                      min_conf_thresh: float = MIN_CONFIDENCE_THRESH,
                      min_num_consistent_views: int = MIN_NUM_CONSISTENT_VIEWS) -> DensePoints:
    """filter_depth on device tensors: depth and confidence (n_valid, H, W) float32 in pm_i order, images_u8 (n_img, h,
    w, 3) uint8 by image index with h >= H and w >= W (the maps cover the top-left corner). One host synchronisation:
    the point count N is read to size the cloud, the same kind as the track count in DsfTracksEstimator.run_arrays."""
    wRc, wtc, intr = valid_cameras(cameras, views)
    f = device.mvs_fuse_depth(depth.contiguous(), confidence.contiguous(), wRc, wtc, intr, views.src_views,
                              max_geo_pixel_thresh, max_geo_depth_thresh, min_conf_thresh, min_num_consistent_views)
    n_points = int(f.counts[:, 2].sum().item())
    points, colors, view_offset = device.mvs_gather_points(f.fused, f.mask, wRc, wtc, intr, images_u8.contiguous(),
                                                           views.pm_to_img, n_points)
    return DensePoints(points, colors, view_offset, f.fused, f.mask, f.counts, f.err)


def filtering_metrics(dense: DensePoints) -> Dict[str, object]:
    """The reference's filtering metrics by name; the reprojection errors as count, mean, min and max."""
    counts, err = dense.counts.cpu().numpy(), dense.err.cpu().numpy()
    hw = max(dense.fused.shape[1] * dense.fused.shape[2], 1)
    n_err = int(counts[:, 3].sum())
    with_err = counts[:, 3] > 0
    return {"geometric_mask_valid_ratios": (counts[:, 0] / hw).tolist(),
            "confidence_mask_valid_ratios": (counts[:, 1] / hw).tolist(),
            "joint_mask_valid_ratios": (counts[:, 2] / hw).tolist(),
            "reprojection_errors": {"count": n_err, "mean": float(err[:, 0].sum() / n_err) if n_err else 0.0,
                                    "min": float(err[with_err, 1].min()) if n_err else 0.0,
                                    "max": float(err[with_err, 2].max()) if n_err else 0.0}}


class MVSDepthFusion(MVSBase):
    """The MVS stage with a pluggable depth estimator (see the module docstring)."""

    def __init__(self, depth_estimator: Callable, max_num_views: int = NUM_VIEWS,
                 max_geo_pixel_thresh: float = MAX_GEOMETRIC_PIXEL_THRESH,
                 max_geo_depth_thresh: float = MAX_GEOMETRIC_DEPTH_THRESH,
                 min_conf_thresh: float = MIN_CONFIDENCE_THRESH,
                 min_num_consistent_views: int = MIN_NUM_CONSISTENT_VIEWS) -> None:
        super().__init__()
        self._depth_estimator = depth_estimator
        self._max_num_views = max_num_views
        self._thresholds = (max_geo_pixel_thresh, max_geo_depth_thresh, min_conf_thresh, min_num_consistent_views)

    def densify_views(self, images_u8: torch.Tensor, cameras, tracks, point: torch.Tensor,
                      track_keep: Optional[torch.Tensor], inlier: Optional[torch.Tensor]
                      ) -> Tuple[DensePoints, MvsViews]:
        """View selection, the depth estimator, fusion. images_u8 (n_img, h, w, 3) uint8 on the device; the maps are h
        and w cropped to multiples of 8 from the top-left corner, as in the reference."""
        _, h, w, _ = images_u8.shape
        H, W = h - h % 8, w - w % 8
        views = select_views_arrays(cameras, tracks, point, track_keep, inlier, self._max_num_views)
        wRc, wtc, intr = valid_cameras(cameras, views)
        crop = images_u8[views.pm_to_img.long(), :H, :W]
        depth, confidence = self._depth_estimator(crop, (wRc, wtc, intr, views.src_views), views.depth_range)
        nv = views.pm_to_img.numel()
        if tuple(depth.shape) != (nv, H, W) or tuple(confidence.shape) != (nv, H, W):
            raise ValueError(f"the depth estimator must return two ({nv}, {H}, {W}) maps, got {tuple(depth.shape)} "
                             f"and {tuple(confidence.shape)}")
        dense = fuse_depth_arrays(depth.to(torch.float32), confidence.to(torch.float32), images_u8, cameras, views,
                                  *self._thresholds)
        return dense, views

    def densify_arrays(self, images_u8: torch.Tensor, result, intrinsics: Optional[torch.Tensor] = None
                       ) -> Tuple[DensePoints, MvsViews]:
        """densify on a MultiViewArrays result directly: ba.wRc, ba.wtc, ba.cam_keep, ba.point, ba.track_keep, tracks
        and triangulated.inlier. intrinsics defaults to the chain's (result.cameras[2])."""
        ba = result.ba
        if ba is None or result.tracks is None or result.triangulated is None or result.cameras is None:
            raise ValueError("densify_arrays needs a chain that reached bundle adjustment: the result's ba, tracks, "
                             "triangulated or cameras is None")
        intr = result.cameras[2] if intrinsics is None else intrinsics
        return self.densify_views(images_u8, (ba.wRc, ba.wtc, intr, ba.cam_keep), result.tracks, ba.point,
                                  ba.track_keep, result.triangulated.inlier)

    def densify(self, images: Dict[int, object], sfm_result) -> Tuple[np.ndarray, np.ndarray, Dict[str, object]]:
        """The reference's signature: images maps image index to Image, sfm_result is a BaData (cameras and tracks).
        Returns points (N, 3), colours (N, 3) uint8 and the filtering metrics."""
        cams = sfm_result.cameras
        if not cams:
            return np.zeros((0, 3)), np.zeros((0, 3), np.uint8), {}
        n_img = max(max(cams), max(images)) + 1
        shapes = {(images[i].height, images[i].width) for i in cams}
        if len(shapes) != 1:
            raise ValueError(f"all images must share one size (resizing is not built), got {sorted(shapes)}")
        (h, w), = shapes
        wRc, wtc = np.tile(np.eye(3), (n_img, 1, 1)), np.zeros((n_img, 3))
        intr, keep = np.tile(np.array([1.0, 0.0, 0.0]), (n_img, 1)), np.zeros(n_img, np.uint8)
        img = np.zeros((n_img, h, w, 3), np.uint8)
        for i, cam in cams.items():
            wRc[i], wtc[i] = geometry.camera_pose(cam)
            K = geometry.calibration_matrix(cam)
            intr[i], keep[i] = (K[0, 0], K[0, 2], K[1, 2]), 1
            a = np.asarray(images[i].value_array)
            img[i] = a[..., :3] if a.ndim == 3 else a[..., None]
        offsets, image, point = [0], [], []
        for track in sfm_result.tracks:
            for k in range(track.numberMeasurements()):
                image.append(int(track.measurement(k)[0]))
            offsets.append(len(image))
            point.append(np.asarray(track.point3(), np.float64).reshape(3))
        dev = upload.cuda_device()
        tracks = _Csr(upload.to_device(np.asarray(offsets, np.int32), dev),
                      upload.to_device(np.asarray(image, np.int32), dev))
        cameras = tuple(upload.to_device(a, dev) for a in (wRc, wtc, intr, keep))
        dense, _ = self.densify_views(upload.to_device(img, dev), cameras, tracks,
                                      upload.to_device(np.asarray(point, np.float64).reshape(-1, 3), dev), None, None)
        return dense.points.cpu().numpy(), dense.colors.cpu().numpy(), filtering_metrics(dense)


class _Csr(NamedTuple):
    offsets: torch.Tensor
    image: torch.Tensor
