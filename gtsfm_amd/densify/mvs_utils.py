"""Utilities of the dense multi-view-stereo stage: counterpart of gtsfm/densify/mvs_utils.py:21-221.

The angle and the Gaussian are the host forms of what gtsfm_mvs_select_views evaluates per measurement pair; the voxel
size and the downsampling run on the device (gtsfm_mvs_voxel_stats, gtsfm_mvs_voxel_keys, gtsfm_mvs_voxel_downsample).
compute_downsampling_psnr and get_voxel_downsampling_metrics' PSNR entry are not built.
"""
import math
from typing import Tuple

import numpy as np
import torch

from gtsfm_amd import device
from gtsfm_amd.common import geometry, upload


def piecewise_gaussian(theta: float, theta_0: float = 5, sigma_1: float = 1, sigma_2: float = 10) -> float:
    """exp(-(theta - theta_0)^2 / (2 sigma^2)) with sigma_1 at or below theta_0 and sigma_2 above it."""
    sigma = sigma_1 if theta <= theta_0 else sigma_2
    return math.exp(-((theta - theta_0) ** 2) / (2 * sigma ** 2))


def calculate_triangulation_angles_in_degrees(camera_1, camera_2, points_3d: np.ndarray) -> np.ndarray:
    """The angles at the 3D points (N, 3) between the rays to the two camera centres, in degrees. A camera is a
    pinhole camera object or its centre as an array."""
    c1, c2 = (np.asarray(c, np.float64).reshape(3) if isinstance(c, np.ndarray) else geometry.camera_pose(c)[1]
              for c in (camera_1, camera_2))
    points_3d = np.asarray(points_3d, np.float64).reshape(-1, 3)
    rays1, rays2 = points_3d - c1, points_3d - c2
    rays1 = rays1 / np.linalg.norm(rays1, axis=1, keepdims=True)
    rays2 = rays2 / np.linalg.norm(rays2, axis=1, keepdims=True)
    return np.rad2deg(np.arccos(np.clip((rays1 * rays2).sum(axis=1), -1, 1)))


def calculate_triangulation_angle_in_degrees(camera_1, camera_2, point_3d: np.ndarray) -> float:
    return float(calculate_triangulation_angles_in_degrees(camera_1, camera_2, np.asarray(point_3d).reshape(1, 3))[0])


def voxel_size_from_stats(stats: np.ndarray, num_points: int, scale: float = 0.02) -> float:
    """scale * sqrt(smallest eigenvalue of the scatter / (N - 1)) from gtsfm_mvs_voxel_stats' 18 numbers; 0 for
    N < 2."""
    if num_points < 2:
        return 0.0
    smallest = float(np.linalg.eigvalsh(np.asarray(stats[3:12], np.float64).reshape(3, 3))[0])
    return scale * math.sqrt(max(smallest, 0.0))


def estimate_minimum_voxel_size_arrays(points: torch.Tensor, scale: float = 0.02) -> Tuple[float, torch.Tensor]:
    """(voxel size, the device statistics) of device points (N, 3) float64. The statistics are read on the host once
    (eighteen numbers) for the 3 x 3 eigvalsh: this synchronises."""
    stats = device.mvs_voxel_stats(points)
    return voxel_size_from_stats(stats.cpu().numpy(), points.shape[0], scale), stats


def estimate_minimum_voxel_size(points: np.ndarray, scale: float = 0.02) -> float:
    points = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    if points.shape[0] < 2:
        return 0
    return estimate_minimum_voxel_size_arrays(upload.to_device(points, upload.cuda_device()), scale)[0]


MAX_VOXELS_PER_AXIS = 2 ** 21  # gtsfm_mvs_voxel_keys packs 21 bits per axis


def check_voxel_extent(stats: np.ndarray, voxel_size: float) -> None:
    """Raises ValueError when the cloud spans MAX_VOXELS_PER_AXIS voxels or more along an axis: the kernel would clamp
    the indices and merge distinct voxels, which Open3D would keep apart. stats is gtsfm_mvs_voxel_stats' 18 numbers."""
    stats = np.asarray(stats, np.float64)
    extent = float(np.max((stats[15:18] - stats[12:15]) / voxel_size)) + 1.5  # the grid starts half a voxel below min
    if not extent < MAX_VOXELS_PER_AXIS:
        raise ValueError(f"the cloud spans {extent:.3g} voxels of size {voxel_size:.3g} along an axis, the voxel keys "
                         f"hold {MAX_VOXELS_PER_AXIS}: choose a larger voxel size")


def downsample_point_cloud_arrays(points: torch.Tensor, rgb: torch.Tensor, voxel_size: float,
                                  stats: torch.Tensor = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """One point per occupied voxel on device tensors points (N, 3) float64 and rgb (N, 3) uint8: the mean position and
    the truncated mean colour, in ascending voxel-key order (Open3D's own order is unspecified). voxel_size <= 0 or an
    empty cloud returns the input; a cloud of 2^21 voxels or more along an axis raises ValueError. The bounds and the
    voxel count are read on the host (two small reads) to check the extent and to slice the result: this synchronises."""
    if voxel_size <= 0 or points.shape[0] == 0:
        return points, rgb
    if stats is None:
        stats = device.mvs_voxel_stats(points)
    check_voxel_extent(stats.cpu().numpy(), voxel_size)
    r = device.mvs_voxel_downsample(points, rgb, stats, voxel_size)
    m = int(r.n_voxels.item())
    return r.points[:m], r.colors[:m]


def downsample_point_cloud(points: np.ndarray, rgb: np.ndarray, voxel_size: float = 0.02
                           ) -> Tuple[np.ndarray, np.ndarray]:
    if voxel_size <= 0 or len(points) == 0:
        return points, rgb
    dev = upload.cuda_device()
    p, c = downsample_point_cloud_arrays(upload.to_device(np.ascontiguousarray(points, np.float64).reshape(-1, 3), dev),
                                         upload.to_device(np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3), dev),
                                         voxel_size)
    return p.cpu().numpy(), c.cpu().numpy()
