"""1DSfM translation averaging on the MI355X.

Drop-in for gtsfm/averaging/translation/averaging_1dsfm.py:68-513 (TranslationAveraging1DSFM): the reference wraps
GTSAM's MFAS (one instance per projection direction, in a Python loop) and TranslationRecovery; here the stage is three
libgtsfm_hip.so calls (gtsfm_transavg_measurements, _mfas, _recover; semantics and the stated deviations in
include/gtsfm_hip.h). Projection directions are drawn on the host from np.random.default_rng(seed) (the reference uses
numpy's global state). SAMPLE_WITH_INPUT_DENSITY (a scipy KDE), pose priors and the ground-truth metrics are not built.

Two forms: run_translation_averaging_arrays takes and returns device tensors (the counts that size the later calls and
the recovery's control scalars reach the host); run_translation_averaging keeps the reference's signature.
"""
from enum import Enum
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from gtsfm_amd import device, native
from gtsfm_amd.averaging.translation.translation_averaging_base import TranslationAveragingBase
from gtsfm_amd.common import geometry, upload
from gtsfm_amd.common.sfm_track import SfmTrack2d

MAX_PROJECTION_DIRECTIONS = 2000
OUTLIER_WEIGHT_THRESHOLD = 0.125
TRACKS_MEASUREMENTS_PER_CAMERA = 12


class TranslationArrays(NamedTuple):
    """run_translation_averaging_arrays' result, device tensors: wti (n_img, 3) float64 and wti_valid (n_img,) uint8;
    landmark (n_selected, 3) and landmark_valid; selected (n_selected,) int32 track ids in selection order; the
    measurement list in use (key (n, 2) int32, dir (n, 3), valid (n,) uint8, n_edges camera slots first) with its
    inlier bytes and outlier_sum (None when reject_outliers is off); stats (10,) float64 in the order of
    native.TA_STATS_FIELDS; counts (4,) int64 of the measurements call."""

    wti: torch.Tensor
    wti_valid: torch.Tensor
    landmark: torch.Tensor
    landmark_valid: torch.Tensor
    selected: torch.Tensor
    key: torch.Tensor
    dir: torch.Tensor
    valid: torch.Tensor
    inlier: torch.Tensor
    outlier_sum: Optional[torch.Tensor]
    stats: torch.Tensor
    counts: torch.Tensor


class TranslationAveraging1DSFM(TranslationAveragingBase):
    """1D-SFM translation averaging with outlier rejection."""

    class ProjectionSamplingMethod(str, Enum):
        """How the projection directions of 1DSfM are sampled."""

        SAMPLE_INPUT_MEASUREMENTS = "SAMPLE_INPUT_MEASUREMENTS"
        SAMPLE_WITH_INPUT_DENSITY = "SAMPLE_WITH_INPUT_DENSITY"
        SAMPLE_WITH_UNIFORM_DENSITY = "SAMPLE_WITH_UNIFORM_DENSITY"

    def __init__(self, robust_measurement_noise: bool = True, use_tracks_for_averaging: bool = True,
                 reject_outliers: bool = True,
                 projection_sampling_method: ProjectionSamplingMethod = ProjectionSamplingMethod.SAMPLE_WITH_UNIFORM_DENSITY,
                 seed: int = 0, pcg_rel_tol: float = 1e-10, pcg_max_iter: int = 2000) -> None:
        super().__init__(robust_measurement_noise)
        self._max_1dsfm_projection_directions = MAX_PROJECTION_DIRECTIONS
        self._outlier_weight_threshold = OUTLIER_WEIGHT_THRESHOLD
        self._reject_outliers = reject_outliers
        self._projection_sampling_method = self.ProjectionSamplingMethod(projection_sampling_method)
        self._use_tracks_for_averaging = use_tracks_for_averaging
        self._seed = int(seed)
        self._pcg_rel_tol = float(pcg_rel_tol)
        self._pcg_max_iter = int(pcg_max_iter)

    def sample_projection_directions(self, measurement_dirs: Optional[torch.Tensor]) -> np.ndarray:
        """(n, 3) float64 projection directions. measurement_dirs: the valid measurements' directions (device), read
        only by SAMPLE_INPUT_MEASUREMENTS."""
        rng = np.random.default_rng(self._seed)
        method = self._projection_sampling_method
        if method == self.ProjectionSamplingMethod.SAMPLE_WITH_UNIFORM_DENSITY:
            d = rng.normal(size=(self._max_1dsfm_projection_directions, 3))
            return d / np.linalg.norm(d, axis=1, keepdims=True)
        if method == self.ProjectionSamplingMethod.SAMPLE_INPUT_MEASUREMENTS:
            n = measurement_dirs.shape[0]
            idx = rng.choice(n, min(n, self._max_1dsfm_projection_directions), replace=False)
            return measurement_dirs[torch.from_numpy(np.sort(idx)).to(measurement_dirs.device)].cpu().numpy()
        raise NotImplementedError("SAMPLE_WITH_INPUT_DENSITY (a scipy KDE over the measurements) is not built")

    def run_translation_averaging_arrays(self, edges: torch.Tensor, i2Ui1: torch.Tensor, wRi: torch.Tensor,
                                         edge_valid: Optional[torch.Tensor] = None,
                                         rot_valid: Optional[torch.Tensor] = None,
                                         track_offsets: Optional[torch.Tensor] = None,
                                         track_img: Optional[torch.Tensor] = None,
                                         track_uv: Optional[torch.Tensor] = None,
                                         intrinsics: Optional[torch.Tensor] = None,
                                         n_tracks_dev: Optional[torch.Tensor] = None, scale_factor: float = 1.0,
                                         measurements_per_camera: int = TRACKS_MEASUREMENTS_PER_CAMERA,
                                         ) -> TranslationArrays:
        """edges (E, 2) int32 = (i1, i2) with i2Ui1 (E, 3) float64, wRi (n_img, 3, 3) float64, the valid masks uint8
        or None, and the track CSR of device.tracks_from_matches (track_offsets, track_img, track_uv, its stats as
        n_tracks_dev) with intrinsics (n_img, 3) float64, or no tracks. Everything stays on the device."""
        native.require_gpu()
        n_img = wRi.numel() // 9
        use_tracks = self._use_tracks_for_averaging and track_offsets is not None
        ms = device.transavg_measurements(edges, i2Ui1, edge_valid, wRi, rot_valid,
                                          track_offsets if use_tracks else None, track_img if use_tracks else None,
                                          track_uv if use_tracks else None, intrinsics if use_tracks else None,
                                          measurements_per_camera, n_tracks_dev=n_tracks_dev if use_tracks else None)
        counts = ms.counts.cpu().numpy()  # sizes the two later calls
        if counts[3] > 0:
            raise ValueError("Camera intrinsics or rotation cannot be None for input track measurements")
        n = ms.n_edges + int(counts[1])
        n_land = int(counts[2])
        key, dirs, valid = ms.key[:n].contiguous(), ms.dir[:n].contiguous(), ms.valid[:n].contiguous()
        osum = None
        inlier = valid
        if self._reject_outliers and counts[0] > 0:
            need_dirs = self._projection_sampling_method == self.ProjectionSamplingMethod.SAMPLE_INPUT_MEASUREMENTS
            proj = self.sample_projection_directions(dirs[valid.bool()] if need_dirs else None)
            proj = upload.to_device(proj, key.device)
            osum, inlier, _ = device.transavg_mfas(key, dirs, valid, n_img + n_land, proj, self._outlier_weight_threshold)
        rec = device.transavg_recover(key, dirs, inlier, n_img, n_land, rot_valid, self._robust_measurement_noise,
                                      scale_factor, self._seed, 0, self._pcg_rel_tol, self._pcg_max_iter)
        return TranslationArrays(rec.wti, rec.wti_valid, rec.landmark, rec.landmark_valid, ms.selected[:n_land], key,
                                 dirs, valid, inlier, osum, rec.stats, ms.counts)

    def run_translation_averaging(self, num_images: int, i2Ui1_dict: Dict[Tuple[int, int], Optional[object]],
                                  wRi_list: List[Optional[object]], tracks_2d: Optional[List[SfmTrack2d]] = None,
                                  intrinsics: Optional[List[Optional[object]]] = None, absolute_pose_priors=(),
                                  i2Ti1_priors=None, scale_factor: float = 1.0, gt_wTi_list=(),
                                  ) -> Tuple[List[Optional[object]], Optional[dict]]:
        """The reference's entry point. i2Ui1_dict values are Unit3, 3-vectors or None; wRi_list entries Rot3, 3 x 3
        arrays or None. Returns the poses (None where no position was computed) and the four count metrics."""
        if i2Ti1_priors or any(p is not None for p in absolute_pose_priors):
            raise NotImplementedError("pose priors are not built into the MI355X translation averaging")
        if self._projection_sampling_method == self.ProjectionSamplingMethod.SAMPLE_WITH_INPUT_DENSITY:
            raise NotImplementedError("SAMPLE_WITH_INPUT_DENSITY (a scipy KDE over the measurements) is not built")
        use_tracks = self._use_tracks_for_averaging and tracks_2d is not None
        if use_tracks and (intrinsics is None or len(intrinsics) != len(wRi_list)):
            raise ValueError("Number of intrinsics must match number of rotations when tracks are provided.")
        pairs = list(i2Ui1_dict.keys())
        metrics = {"num_total_1dsfm_measurements": sum(1 for v in i2Ui1_dict.values() if v is not None),
                   "num_inlier_1dsfm_measurements": 0, "num_outlier_1dsfm_measurements": 0,
                   "num_translations_estimated": 0}
        metrics["num_outlier_1dsfm_measurements"] = metrics["num_total_1dsfm_measurements"]
        if not pairs:
            return [None] * num_images, metrics
        dev = upload.cuda_device()
        u = np.zeros((len(pairs), 3))
        ev = np.zeros(len(pairs), np.uint8)
        for k, p in enumerate(pairs):
            v = i2Ui1_dict[p]
            if v is not None:
                u[k] = geometry.unit_vector(v) if hasattr(v, "point3") else np.asarray(v, np.float64).reshape(3)
                ev[k] = 1
        R = np.tile(np.eye(3), (num_images, 1, 1))
        rv = np.zeros(num_images, np.uint8)
        for i, r in enumerate(wRi_list):
            if r is not None:
                R[i] = geometry.rotation_matrix(r)
                rv[i] = 1
        track_args = {}
        if use_tracks and len(tracks_2d) > 0:
            lens = [t.number_measurements() for t in tracks_2d]
            off = np.zeros(len(lens) + 1, np.int32)
            np.cumsum(lens, out=off[1:])
            img = np.array([m.i for t in tracks_2d for m in t.measurements], np.int32)
            uv = np.array([np.asarray(m.uv, np.float64) for t in tracks_2d for m in t.measurements]).reshape(-1, 2)
            K = np.tile(np.array([1.0, 0.0, 0.0]), (num_images, 1))
            for i, c in enumerate(intrinsics):
                if c is not None:
                    K[i] = geometry.calibration_params(c)
            track_args = dict(track_offsets=off, track_img=img, track_uv=uv, intrinsics=K)
        edges = np.asarray(pairs, np.int32).reshape(-1, 2)
        res = self.run_translation_averaging_arrays(
            *(upload.to_device(a, dev) for a in (edges, u, R, ev, rv)), scale_factor=scale_factor,
            **{k: upload.to_device(a, dev) for k, a in track_args.items()})
        wti, ok = res.wti.cpu().numpy(), res.wti_valid.cpu().numpy()
        inl = int(res.inlier[: len(pairs)].sum().item())
        metrics["num_inlier_1dsfm_measurements"] = inl
        metrics["num_outlier_1dsfm_measurements"] = metrics["num_total_1dsfm_measurements"] - inl
        metrics["num_translations_estimated"] = int(ok.sum())
        poses = [geometry.Pose3(geometry.Rot3(R[i]), wti[i]) if ok[i] else None for i in range(num_images)]
        return poses, metrics
