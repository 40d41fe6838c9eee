"""Data association: 3D tracks from 2D tracks and cameras (reference gtsfm/data_association/data_assoc.py:40-273).

Only the triangulation step is here. run_triangulation keeps the reference's signature and its three lists, from one
gtsfm_triangulate_tracks launch instead of one dask task per batch of tracks; run_triangulation_arrays is the array
form for the device-resident chain. assemble_gtsfm_data_from_tracks (GtsfmData, the largest connected component of
cameras and the metrics, data_assoc.py:76-209) is out of scope and stays with the reference.
"""
from typing import Dict, List, NamedTuple, Optional, Tuple

import torch

from gtsfm_amd.common.sfm_track import SfmTrack, SfmTrack2d
from gtsfm_amd.data_association.dsf_tracks_estimator import Tracks2d
from gtsfm_amd.data_association.point3d_initializer import (
    Point3dInitializer,
    Triangulated,
    TriangulationExitCode,
    TriangulationOptions,
)


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

    def run_triangulation_arrays(self, cameras: Dict[int, object], tracks: Tracks2d, seed: int = 0,
                                 n_tracks_dev: Optional[torch.Tensor] = None):
        """(Triangulated, valid): the per-track arrays of Point3dInitializer.triangulate_arrays and valid (T,) bool =
        exit code SUCCESS with at least min_track_len inlier measurements (validate_track). numpy or device tensors, as
        the tracks; nothing is copied to the host for device tensors."""
        r: Triangulated = Point3dInitializer(cameras, self.triangulation_options, seed).triangulate_arrays(
            tracks, n_tracks_dev=n_tracks_dev)
        if isinstance(r.exit_code, torch.Tensor):
            T = r.exit_code.numel()
            csum = torch.zeros(r.inlier.numel() + 1, dtype=torch.int64, device=r.inlier.device)
            csum[1:] = torch.cumsum(r.inlier.to(torch.int64), 0)
            off = tracks.offsets.to(torch.int64)[: T + 1]
            kept = csum[off[1:]] - csum[off[:-1]]
            return r, (r.exit_code == 0) & (kept >= self.min_track_len)
        import numpy as np

        csum = np.concatenate([[0], np.cumsum(r.inlier.astype(np.int64))])
        off = np.asarray(tracks.offsets, np.int64)
        kept = csum[off[1:]] - csum[off[:-1]]
        return r, (r.exit_code == 0) & (kept >= self.min_track_len)
