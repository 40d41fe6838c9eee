"""2D feature tracks from pairwise correspondences on the MI355X: a disjoint-set forest keyed on (image, keypoint).

Drop-in for gtsfm/data_association/dsf_tracks_estimator.py:25-93 and cpp_dsf_tracks_estimator.py:26-88: every
correspondence row merges its two (i, k) nodes, every connected component is a candidate track, and a component with
two keypoints of one image is discarded. The reference merges row by row in a Python loop (or in gtsam); here one
gtsfm_tracks_from_matches call (libgtsfm_hip.so) runs a lock-free union-find with one lane per row and groups the
result on the device.

Track order is canonical: tracks by ascending smallest (i, k), measurements by ascending (i, k) inside a track. The
reference's order follows gtsam's internal representative, and its SfmTrack2d.__eq__ ignores measurement order.
"""
import logging
import time
from typing import Dict, List, NamedTuple, Optional, Tuple, Union

import numpy as np
import torch

from gtsfm_amd import device
from gtsfm_amd.common import upload
from gtsfm_amd.common.keypoints import Keypoints
from gtsfm_amd.common.sfm_track import SfmMeasurement, SfmTrack2d
from gtsfm_amd.data_association.tracks_estimator_base import TracksEstimatorBase

logger = logging.getLogger(__name__)

ArrayLike = Union[np.ndarray, torch.Tensor]

STATS_FIELDS = ("n_tracks", "n_measurements", "n_components", "n_erroneous", "n_bad_rows")


class Tracks2d(NamedTuple):
    """Tracks as arrays: track t owns measurements offsets[t] .. offsets[t + 1] of image / keypoint / uv.

    offsets (n_tracks + 1,) int32, image (n_measurements,) int32, keypoint (n_measurements,) int32, uv
    (n_measurements, 2) float32 or None (no kp_xy given), stats (5,) int64 in the order of STATS_FIELDS."""

    offsets: ArrayLike
    image: ArrayLike
    keypoint: ArrayLike
    uv: Optional[ArrayLike]
    stats: ArrayLike


class DsfTracksEstimator(TracksEstimatorBase):
    """Estimates tracks with a disjoint-set forest built on the GPU."""

    def run_arrays(self, pairs: ArrayLike, offsets: ArrayLike, v_corr: ArrayLike, kp_count: ArrayLike, kmax: int,
                   valid: Optional[ArrayLike] = None, kp_xy: Optional[ArrayLike] = None) -> Tracks2d:
        """Tracks of a CSR of correspondences: pairs (P, 2) image indices (any order, i1 == i2 and repeats allowed),
        offsets (P + 1,), v_corr (rows, 2) keypoint indices (k1, k2) with pair p owning rows offsets[p] ..
        offsets[p + 1], kp_count (n_img,) keypoints per image, kmax >= max(kp_count), valid (P,) bool or None, kp_xy
        (n_img, kmax, 2) float32 or None. Rows of v_corr past offsets[P] are ignored, so the buffer may be larger than
        its contents. A row naming an image outside [0, n_img) or a keypoint >= kp_count[i] is skipped and counted in
        stats[4].

        This is the layout the batched front-end leaves on the device, and the chain needs no host copy:

            offsets, v_corr, isp_ok = device.compact_verified(...)             # or HostResults' arrays, uploaded
            keep, _, _ = CycleConsistentRotationViewGraphEstimator(...).run_arrays(pairs, R, valid=ok, num_images=n)
            tracks = DsfTracksEstimator().run_arrays(pairs, offsets, v_corr, kp_count, kmax,
                                                     valid=keep & (isp_ok != 0), kp_xy=kp_xy)

        The result is of the kind of `pairs`: numpy in gives numpy out, a torch tensor in gives torch tensors on that
        tensor's device (a CPU tensor is copied to the GPU and the results back, like numpy). With `pairs` on the GPU
        the only host synchronisation is the one read of `stats` that sizes the returned slices."""
        is_tensor = isinstance(pairs, torch.Tensor)
        dev = upload.cuda_device(pairs)
        pairs_d = upload.to_device(pairs, dev, torch.int32, (-1, 2))
        P = pairs_d.shape[0]
        offsets_d = upload.to_device(offsets, dev, torch.int32, (-1,))
        if offsets_d.numel() < P + 1:
            raise ValueError(f"offsets has {offsets_d.numel()} entries for {P} pairs")
        # keypoint indices: a uint32 array is taken as the int32 tensor the kernel reads as uint32
        v_corr_d = upload.to_device(v_corr, dev, torch.int32, (-1, 2))
        kp_count_d = upload.to_device(kp_count, dev, torch.int32, (-1,))
        valid_d = None if valid is None else upload.mask_to_device(valid, dev, P)
        kp_xy_d = None if kp_xy is None else upload.to_device(kp_xy, dev, torch.float32,
                                                              (kp_count_d.numel(), int(kmax), 2))
        t_off, t_img, t_kp, t_uv, stats = device.tracks_from_matches(pairs_d, offsets_d, v_corr_d, kp_count_d, int(kmax),
                                                                     valid=valid_d, kp_xy=kp_xy_d)
        stats_h = stats.cpu()  # the one synchronisation: the counts size the slices below
        n_tracks, n_meas = int(stats_h[0]), int(stats_h[1])
        out = (t_off[: n_tracks + 1], t_img[:n_meas], t_kp[:n_meas], None if t_uv is None else t_uv[:n_meas])
        if is_tensor:
            to = pairs.device
            return Tracks2d(*(None if a is None else a.to(to) for a in out), stats.to(to))
        return Tracks2d(*(None if a is None else a.cpu().numpy() for a in out), stats_h.numpy())

    def run(self, matches_dict: Dict[Tuple[int, int], np.ndarray], keypoints_list: List[Keypoints]) -> List[SfmTrack2d]:
        """The reference's run(): matches_dict maps (i1, i2) to (K, 2) rows (k1, k2); keypoints_list holds the
        Keypoints of every image (None = an image without detections).

        Raises ValueError when some coordinates array is not 2-D (cpp_dsf_tracks_estimator.py:50-61) and IndexError
        when a row names an image or keypoint that does not exist, where the reference's list indexing would
        (dsf_tracks_estimator.py:76); both before the GPU is touched. Measurements carry keypoints_list's own
        coordinates (their dtype included), indexed on the host by the kernel's (image, keypoint) output."""
        start = time.time()
        wrong = [f"i={i}: shape={kps.coordinates.shape}," for i, kps in enumerate(keypoints_list)
                 if kps is not None and kps.coordinates.ndim != 2]
        if wrong:
            raise ValueError("Dimensions for Keypoint coordinates incorrect. Array needs to be 2D, but found "
                             + " ".join(wrong))
        n_img = len(keypoints_list)
        kp_count = np.array([0 if kps is None else len(kps.coordinates) for kps in keypoints_list], dtype=np.int32)
        pairs, counts, rows = [], [], []
        for (i1, i2), corr in matches_dict.items():
            corr = np.asarray(corr).reshape(-1, 2).astype(np.int64)
            for i, col in ((int(i1), corr[:, 0]), (int(i2), corr[:, 1])):
                if not 0 <= i < n_img:
                    raise IndexError(f"pair ({i1}, {i2}): image {i} is not in keypoints_list ({n_img} images)")
                if len(col) and (col.min() < 0 or col.max() >= kp_count[i]):
                    raise IndexError(f"pair ({i1}, {i2}): keypoint index out of range for image {i} "
                                     f"({kp_count[i]} keypoints)")
            pairs.append((int(i1), int(i2)))
            counts.append(len(corr))
            rows.append(corr)
        if not pairs or sum(counts) == 0:
            logger.info("DSF Union-Find: nan% of tracks discarded from multiple obs. in a single image.")
            return []
        offsets = np.zeros(len(pairs) + 1, dtype=np.int64)
        np.cumsum(counts, out=offsets[1:])
        tracks = self.run_arrays(np.array(pairs, dtype=np.int32), offsets.astype(np.int32),
                                 np.concatenate(rows).astype(np.int32), kp_count, max(int(kp_count.max()), 1))
        track_2d_list = []
        for t in range(len(tracks.offsets) - 1):
            lo, hi = int(tracks.offsets[t]), int(tracks.offsets[t + 1])
            track_2d_list.append(SfmTrack2d([
                SfmMeasurement(int(i), keypoints_list[int(i)].coordinates[int(k)])
                for i, k in zip(tracks.image[lo:hi], tracks.keypoint[lo:hi])]))
        n_components, n_erroneous = int(tracks.stats[2]), int(tracks.stats[3])
        erroneous_pct = n_erroneous / n_components * 100 if n_components > 0 else float("nan")
        logger.info("DSF Union-Find: %.2f%% of tracks discarded from multiple obs. in a single image.", erroneous_pct)
        logger.info("DsfTracksEstimator took %.2f sec. to estimate %d tracks.", time.time() - start, len(track_2d_list))
        return track_2d_list


CppDsfTracksEstimator = DsfTracksEstimator  # the reference's other name for the same computation


def get_2d_tracks(corr_idxs_dict: Dict[Tuple[int, int], np.ndarray],
                  keypoints_list: List[Keypoints]) -> List[SfmTrack2d]:
    """The 2D tracks of the view graph's correspondences (gtsfm/multi_view_optimizer.py:195-199)."""
    return CppDsfTracksEstimator().run(corr_idxs_dict, keypoints_list)
