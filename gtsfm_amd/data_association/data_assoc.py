"""Data association: 3D tracks from 2D tracks and cameras (reference gtsfm/data_association/data_assoc.py:40-273).

run_triangulation keeps the reference's signature and its three lists, from one gtsfm_triangulate_tracks launch instead
of one dask task per batch of tracks; run_triangulation_arrays is the array form for the device-resident chain.
assemble_arrays is the array form of assemble_gtsfm_data_from_tracks (data_assoc.py:76-209): the valid tracks, the
largest connected component of cameras they join and the tracks wholly inside it, from one gtsfm_assemble_ba_input
call, as the masks BundleAdjustmentOptimizer.run_ba_arrays takes. Of its metrics the three counts are derived from the
call's statistics (assemble_metrics); the histograms and the exit-code table against ground-truth cameras stay with the
reference, as do GtsfmData itself and the track-patch visualisation.
"""
from typing import Dict, List, NamedTuple, Optional, Tuple, Union

import numpy as np
import torch

from gtsfm_amd import device, native
from gtsfm_amd.common import upload
from gtsfm_amd.common.sfm_track import SfmTrack, SfmTrack2d
from gtsfm_amd.data_association.dsf_tracks_estimator import Tracks2d
from gtsfm_amd.data_association.point3d_initializer import (
    DeviceCameras,
    Point3dInitializer,
    Triangulated,
    TriangulationExitCode,
    TriangulationOptions,
)

ArrayLike = Union[np.ndarray, torch.Tensor]


class BaInputArrays(NamedTuple):
    """assemble_arrays' result (numpy or torch, as the tracks given): cam_keep (n_img,) and track_keep (T,) uint8,
    track_len (T,) int32 (the inlier count of a kept track, else 0: the reference's 3d_tracks_length), stats (6,)
    int64 in the order of native.BA_INPUT_STATS_FIELDS."""

    cam_keep: ArrayLike
    track_keep: ArrayLike
    track_len: ArrayLike
    stats: ArrayLike


def assemble_metrics(stats: ArrayLike, num_tracks_2d: int) -> Dict[str, float]:
    """The three count metrics of data_assoc.py:169-195 from BaInputArrays.stats (read on the host)."""
    s = dict(zip(native.BA_INPUT_STATS_FIELDS, (int(v) for v in torch.as_tensor(stats).cpu().tolist())))
    return {"accepted_tracks_ratio": s["tracks_kept"] / num_tracks_2d if num_tracks_2d else float("nan"),
            "num_accepted_tracks": s["tracks_kept"], "number_cameras": s["cameras_kept"]}


class DataAssociation(NamedTuple):
    """min_track_len: the fewest measurements a triangulated track must keep to be valid (data_assoc.py:72-74);
    triangulation_options: mode, thresholds and RANSAC parameters."""

    min_track_len: int
    triangulation_options: TriangulationOptions

    def validate_track(self, sfm_track: Optional[SfmTrack]) -> bool:
        """The reference's __validate_track: a track that exists and keeps at least min_track_len measurements."""
        return sfm_track is not None and sfm_track.numberMeasurements() >= self.min_track_len

    def run_triangulation(self, cameras: Dict[int, object], tracks_2d: List[SfmTrack2d], seed: int = 0,
                          ) -> Tuple[List[Optional[SfmTrack]], List[Optional[float]], List[TriangulationExitCode]]:
        """(sfm_tracks, avg_track_reproj_errors, triangulation_exit_codes), one entry per 2D track."""
        results = Point3dInitializer(cameras, self.triangulation_options, seed).triangulate_list(tracks_2d)
        return [r[0] for r in results], [r[1] for r in results], [r[2] for r in results]

    def run_triangulation_arrays(self, cameras: Union[Dict[int, object], DeviceCameras], tracks: Tracks2d,
                                 seed: int = 0, n_tracks_dev: Optional[torch.Tensor] = None):
        """(Triangulated, valid): the per-track arrays of Point3dInitializer.triangulate_arrays and valid (T,) bool =
        exit code SUCCESS with at least min_track_len inlier measurements (validate_track). numpy or device tensors, as
        the tracks; nothing is copied to the host for device tensors. cameras is {image index: camera or None} or the
        tuple of device tensors (wRc, wtc, intrinsics, cam_valid), which is used as it is."""
        r: Triangulated = Point3dInitializer(cameras, self.triangulation_options, seed).triangulate_arrays(
            tracks, n_tracks_dev=n_tracks_dev)
        if isinstance(r.exit_code, torch.Tensor):
            T = r.exit_code.numel()
            csum = torch.zeros(r.inlier.numel() + 1, dtype=torch.int64, device=r.inlier.device)
            csum[1:] = torch.cumsum(r.inlier.to(torch.int64), 0)
            off = tracks.offsets.to(torch.int64)[: T + 1]
            kept = csum[off[1:]] - csum[off[:-1]]
            return r, (r.exit_code == 0) & (kept >= self.min_track_len)

        csum = np.concatenate([[0], np.cumsum(r.inlier.astype(np.int64))])
        off = np.asarray(tracks.offsets, np.int64)
        kept = csum[off[1:]] - csum[off[:-1]]
        return r, (r.exit_code == 0) & (kept >= self.min_track_len)

    def assemble_arrays(self, tracks: Tracks2d, triangulated: Triangulated, valid: ArrayLike, cam_valid: ArrayLike,
                        extra_camera_edges: Optional[ArrayLike] = None,
                        n_tracks_dev: Optional[torch.Tensor] = None) -> BaInputArrays:
        """The bundle-adjustment input of assemble_gtsfm_data_from_tracks (data_assoc.py:123-160) as masks: cam_keep,
        the valid cameras in the largest connected component of the cameras that the valid tracks join, and
        track_keep, the valid tracks whose inlier measurements all lie in kept cameras. tracks, triangulated and valid
        are what run_triangulation_arrays took and returned; cam_valid (n_img,) marks the cameras init_cameras gave;
        extra_camera_edges (n, 2) are the reference's keys of the relative-pose priors.

        The reference skips CHEIRALITY_FAILURE tracks before it validates (:134-135). valid already requires exit code
        SUCCESS, so no track with another exit code is accepted and the exit code is not tested again here.
        numpy in gives numpy out; device tensors in give device tensors out, with no host copy or synchronisation."""
        is_tensor = isinstance(tracks.offsets, torch.Tensor)
        dev = upload.cuda_device(tracks.offsets)
        T = int(triangulated.exit_code.shape[0])
        cam_valid_d = upload.mask_to_device(cam_valid, dev, -1)
        edges = None
        if extra_camera_edges is not None and len(extra_camera_edges) > 0:
            edges = upload.to_device(extra_camera_edges, dev, torch.int32, (-1, 2))
        r = device.assemble_ba_input(
            upload.to_device(tracks.offsets, dev, torch.int32, (-1,)),
            upload.to_device(tracks.image, dev, torch.int32, (-1,)), upload.mask_to_device(valid, dev, -1),
            upload.to_device(triangulated.inlier, dev, torch.uint8, (-1,)), cam_valid_d, cam_valid_d.numel(), edges,
            n_tracks=T, n_tracks_dev=n_tracks_dev)
        out = (r.cam_keep, r.track_keep, r.track_len, r.stats)
        if is_tensor:
            return BaInputArrays(*(a.to(tracks.offsets.device) for a in out))
        return BaInputArrays(*(a.cpu().numpy() for a in out))
