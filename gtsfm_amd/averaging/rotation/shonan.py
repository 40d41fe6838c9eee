"""Shonan rotation averaging on the MI355X.

Drop-in for gtsfm/averaging/rotation/shonan.py:38-199 (ShonanRotationAveraging): the reference wraps GTSAM's
ShonanAveraging3; here the stage is one libgtsfm_hip.so call (gtsfm_rotavg_shonan; semantics and the stated deviations
in include/gtsfm_hip.h). The call keeps the largest connected component itself and renumbers the cameras, so the
reference's old_to_new_idxes wrapper (:183-197) has no counterpart here. Dask, the metrics and the UI metadata are not
built.

Two forms: run_rotation_averaging_arrays takes the verifier's edge tensor and the view graph's keep mask and returns
device tensors that pass straight into TranslationAveraging1DSFM.run_translation_averaging_arrays;
run_rotation_averaging keeps the reference's signature.
"""
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from gtsfm_amd import device, native
from gtsfm_amd.averaging.rotation.rotation_averaging_base import RotationAveragingBase
from gtsfm_amd.common import geometry, upload
from gtsfm_amd.common.pose_prior import PosePrior

_DEFAULT_TWO_VIEW_ROTATION_SIGMA = 1.0


class RotationArrays(NamedTuple):
    """run_rotation_averaging_arrays' result, device tensors: wRi (n_img, 3, 3) float64, rot_valid (n_img,) uint8 and
    stats (12,) float64 in the order of native.RA_STATS_FIELDS."""

    wRi: torch.Tensor
    rot_valid: torch.Tensor
    stats: torch.Tensor


class ShonanRotationAveraging(RotationAveragingBase):
    """Performs Shonan rotation averaging."""

    def __init__(self, two_view_rotation_sigma: float = _DEFAULT_TWO_VIEW_ROTATION_SIGMA, seed: int = 0) -> None:
        self._two_view_rotation_sigma = float(two_view_rotation_sigma)
        self._p_min = 5
        self._p_max = 30
        self._seed = int(seed)

    def run_rotation_averaging_arrays(self, edges: torch.Tensor, i2Ri1: torch.Tensor,
                                      edge_valid: Optional[torch.Tensor], num_images: int,
                                      prior_edges: Optional[torch.Tensor] = None,
                                      prior_i1Ri2: Optional[torch.Tensor] = None,
                                      prior_sigma: Optional[torch.Tensor] = None,
                                      wRi_init: Optional[torch.Tensor] = None) -> RotationArrays:
        """edges (E, 2) int32 = (i1, i2) with i2Ri1 (E, 3, 3) float64 and edge_valid (E,) uint8 or None, as the
        verifier and the view-graph filter leave them; optionally priors (i1, i2) with i1Ri2 and their sigmas.
        Everything stays on the device; the staircase's control scalars reach the host."""
        native.require_gpu()
        # (i1, i2) -> i2Ri1 is the edge a = i2, b = i1 (shonan.py:75); a prior (i1, i2) -> i1Ri2 is a = i1, b = i2 (:97)
        ab = edges.flip(1).contiguous()
        aRb = i2Ri1.reshape(-1, 3, 3)
        kappa = None
        if prior_edges is not None and prior_edges.numel() > 0:
            n_e = ab.shape[0]
            ab = torch.cat([ab, prior_edges.to(torch.int32)]).contiguous()
            aRb = torch.cat([aRb, prior_i1Ri2.reshape(-1, 3, 3)])
            kappa = torch.cat([torch.full((n_e,), 1.0 / self._two_view_rotation_sigma ** 2, dtype=torch.float64,
                                          device=ab.device), 1.0 / prior_sigma.to(torch.float64) ** 2]).contiguous()
            if edge_valid is not None:
                edge_valid = torch.cat([edge_valid, torch.ones(prior_edges.shape[0], dtype=torch.uint8,
                                                               device=ab.device)]).contiguous()
        elif self._two_view_rotation_sigma != 1.0:
            kappa = torch.full((ab.shape[0],), 1.0 / self._two_view_rotation_sigma ** 2, dtype=torch.float64,
                               device=ab.device)
        res = device.rotavg_shonan(ab, aRb.contiguous(), kappa, edge_valid, num_images, wRi_init, self._seed,
                                   self._p_min, self._p_max)
        return RotationArrays(res.wRi, res.rot_valid, res.stats)

    def run_rotation_averaging(self, num_images: int, i2Ri1_dict: Dict[Tuple[int, int], Optional[object]],
                               i1Ti2_priors: Dict[Tuple[int, int], PosePrior]) -> List[Optional[object]]:
        """The reference's entry point. i2Ri1_dict values are Rot3, 3 x 3 arrays or None (skipped); returns Rot3 per
        image, None where the camera has no measurement, lies outside the largest component, or nothing was computed."""
        if len(i2Ri1_dict) == 0:
            return [None] * num_images
        pairs = [k for k, v in i2Ri1_dict.items() if v is not None]
        R = [geometry.rotation_matrix(i2Ri1_dict[k]) for k in pairs]
        p_pairs = list(i1Ti2_priors.keys())
        p_R = [geometry.rotation_matrix(i1Ti2_priors[k].value.rotation()) for k in p_pairs]
        p_sigma = [float(np.sqrt(np.average(np.diag(i1Ti2_priors[k].covariance), axis=None))) for k in p_pairs]
        if not pairs and not p_pairs:
            return [None] * num_images
        dev = upload.cuda_device()
        res = self.run_rotation_averaging_arrays(
            upload.to_device(np.asarray(pairs, np.int32), dev, shape=(-1, 2)),
            upload.to_device(np.asarray(R, np.float64), dev, shape=(-1, 3, 3)), None, num_images,
            upload.to_device(np.asarray(p_pairs, np.int32), dev, shape=(-1, 2)) if p_pairs else None,
            upload.to_device(np.asarray(p_R, np.float64), dev, shape=(-1, 3, 3)) if p_pairs else None,
            upload.to_device(np.asarray(p_sigma, np.float64), dev) if p_pairs else None)
        status = int(res.stats[11].item())
        if status == native.RA_STATUS_UNCERTIFIED:
            raise RuntimeError("Shonan rotation averaging reached p_max without an optimality certificate")
        wRi, ok = res.wRi.cpu().numpy(), res.rot_valid.cpu().numpy()
        return [geometry.Rot3(wRi[i]) if ok[i] else None for i in range(num_images)]
