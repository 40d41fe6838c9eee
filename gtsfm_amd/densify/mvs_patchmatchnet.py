"""MVSPatchmatchNet: the reference's dense-MVS class (gtsfm/densify/mvs_patchmatchnet.py:55-199) on the HIP
PatchmatchNet: MVSDepthFusion with PatchmatchNetDepthEstimator as its depth estimator.

The reference reads its checkpoint from a fixed path inside its source tree; here the path is a constructor argument
(the checkpoint is not shipped) and a state dict or packed blob can be given instead.
"""
import os
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from gtsfm_amd.densify import mvs_depth_fusion as mdf
from gtsfm_amd.densify.patchmatchnet import PatchmatchNetDepthEstimator


def load_checkpoint(path: str) -> Dict[str, torch.Tensor]:
    """The state dict of a PatchmatchNet checkpoint: the reference's {"model": state_dict} file or a bare state dict."""
    if not os.path.isfile(path):
        raise FileNotFoundError(f"PatchmatchNet checkpoint not found: {path} (the pretrained weights are not shipped; "
                                "pass the path of model_000007.ckpt, or weights=)")
    ckpt = torch.load(path, map_location="cpu")
    return ckpt["model"] if isinstance(ckpt, dict) and "model" in ckpt else ckpt


class MVSPatchmatchNet(mdf.MVSDepthFusion):
    """Dense point cloud from bundle-adjusted cameras and tracks with PatchmatchNet depth maps."""

    def __init__(self, checkpoint_path: Optional[str] = None, weights=None, seed: int = 0) -> None:
        if (checkpoint_path is None) == (weights is None):
            raise ValueError("give exactly one of checkpoint_path and weights")
        super().__init__(PatchmatchNetDepthEstimator(load_checkpoint(checkpoint_path) if weights is None else weights,
                                                     seed))

    def densify(self, images: Dict[int, object], sfm_result, max_num_views: int = mdf.NUM_VIEWS,
                max_geo_pixel_thresh: float = mdf.MAX_GEOMETRIC_PIXEL_THRESH,
                max_geo_depth_thresh: float = mdf.MAX_GEOMETRIC_DEPTH_THRESH,
                min_conf_thresh: float = mdf.MIN_CONFIDENCE_THRESH,
                min_num_consistent_views: float = mdf.MIN_NUM_CONSISTENT_VIEWS, num_workers: int = 0
                ) -> Tuple[np.ndarray, np.ndarray, Dict[str, object]]:
        """The reference's signature. num_workers must be 0, as there (no data loader exists here at all)."""
        if num_workers != 0:
            raise ValueError("num_workers must be 0: there is no data loader to parallelise")
        self._max_num_views = max_num_views
        self._thresholds = (max_geo_pixel_thresh, max_geo_depth_thresh, min_conf_thresh, int(min_num_consistent_views))
        return super().densify(images, sfm_result)
