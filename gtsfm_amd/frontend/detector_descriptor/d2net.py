"""D2-Net detector-descriptor on the MI355X.

Drop-in for gtsfm/frontend/detector_descriptor/d2net.py:32-88 (D2NetDetDesc): same constructor (max_keypoints,
model_path, use_cuda), same outputs: Keypoints(coordinates (N, 2) float32 (x, y), responses=scores) and (N, 512)
float32 unit descriptors, the `max_keypoints` highest scores in descending order. The single-scale path the reference
runs (USE_MULTISCALE False): preprocessing, the VGG16 trunk to conv4_3 with its dilated conv4, hard detection,
handcrafted localisation, bilinear description and the top-k (thirdparty/d2net/lib/model_test.py, pyramid.py,
utils.py) are one call into libgtsfm_hip.so (gtsfm_d2net_batched).

Weights: the checkpoint at `model_path` (d2_tf.pth: {"model": state_dict} with the keys
dense_feature_extraction.model.{0,2,5,7,10,12,14,17,19,21}.{weight,bias}), loaded with torch.load(weights_only=True),
or a state dict passed in directly as `state_dict` (name -> array).

The one deviation: an image over MAX_EDGE_PX or MAX_SUM_EDGES_PX is downsampled by the reference with
scipy.misc.imresize (d2net.py:113-118), which scipy no longer has. Here it is resized on the device with
torch.nn.functional.interpolate(mode="bilinear", antialias=True) and rounded to uint8, to the size the reference
would produce: the scale factor applied to both axes and truncated, as PIL does for imresize's fractional size;
fact_i, fact_j are the reference's ratios of the original to the resized shape. Images within the limits go through
untouched.
"""
from pathlib import Path
from typing import Dict, List, Optional, Tuple, Union

import numpy as np
import torch

from gtsfm_amd import device, native
from gtsfm_amd.common.image import Image
from gtsfm_amd.common.keypoints import Keypoints
from gtsfm_amd.frontend.detector_descriptor.detector_descriptor_base import DetectorDescriptorBase

MAX_EDGE_PX = 1600
MAX_SUM_EDGES_PX = 2800
MODEL_PATH = Path("thirdparty/d2net/weights/d2_tf.pth")

# (index in dense_feature_extraction.model, cin, cout): the packed blob layout of include/gtsfm_hip.h
D2NET_CONVS = [(0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256),
               (17, 256, 512), (19, 512, 512), (21, 512, 512)]
_PREFIX = "dense_feature_extraction.model"


def pack_d2net_weights(state_dict: Dict[str, np.ndarray]) -> np.ndarray:
    """Reference state dict (weight (cout, cin, 3, 3), bias) -> the packed fp32 blob: per convolution W[9][cin][cout]
    (W[ky * 3 + kx][ci][co] = weight[co][ci][ky][kx]) followed by bias[cout]."""
    parts = []
    for idx, cin, cout in D2NET_CONVS:
        w = np.asarray(state_dict[f"{_PREFIX}.{idx}.weight"], np.float32)
        b = np.asarray(state_dict[f"{_PREFIX}.{idx}.bias"], np.float32)
        assert w.shape == (cout, cin, 3, 3) and b.shape == (cout,), (idx, w.shape, b.shape)
        parts += [np.ascontiguousarray(w.transpose(2, 3, 1, 0)).ravel(), b]
    return np.concatenate(parts)


def load_state_dict(model_path: Union[Path, str]) -> Dict[str, np.ndarray]:
    ckpt = torch.load(str(model_path), map_location="cpu", weights_only=True)
    return {k: v.numpy() for k, v in ckpt["model"].items()}


def resized_shape(H: int, W: int, max_edge_px: int = MAX_EDGE_PX,
                  max_sum_edges_px: int = MAX_SUM_EDGES_PX) -> Tuple[int, int, float, float]:
    """resize_image's arithmetic (d2net.py:111-122) for an (H, W, 3) image: (H1, W1, fact_i, fact_j). The limit on
    the longer edge is applied first, the limit on the sum to its result; each scale is applied to both axes and
    truncated (imresize with a fractional size)."""
    h, w = H, W
    if max(h, w, 3) > max_edge_px:
        s = max_edge_px / max(h, w, 3)
        h, w = int(h * s), int(w * s)
    if h + w > max_sum_edges_px:
        s = max_sum_edges_px / (h + w)
        h, w = int(h * s), int(w * s)
    return h, w, H / h, W / w


class D2NetDetDesc(DetectorDescriptorBase):
    """D2-Net (single scale) computed by HIP kernels."""

    def __init__(self, max_keypoints: int = 5000, model_path: Union[Path, str] = MODEL_PATH, use_cuda: bool = True,
                 state_dict: Optional[Dict[str, np.ndarray]] = None) -> None:
        super().__init__(max_keypoints=max_keypoints)
        self.model_path = model_path
        self.use_cuda = use_cuda
        if state_dict is None:
            if not Path(model_path).is_file():
                raise FileNotFoundError(
                    f"D2-Net checkpoint not found at {model_path}: pass model_path= (the reference's d2_tf.pth) or "
                    f"state_dict=")
            state_dict = load_state_dict(model_path)
        self._packed = pack_d2net_weights(state_dict)  # host copy: travels with a pickle
        self._blob: Optional[torch.Tensor] = None

    def __getstate__(self):
        s = self.__dict__.copy()
        s["_blob"] = None  # device memory is re-created per process
        return s

    def weights(self) -> torch.Tensor:
        if self._blob is None:
            native.require_gpu()
            self._blob = torch.from_numpy(self._packed).to(torch.device("cuda"))
        return self._blob

    def extract_batch(self, arrays: List[np.ndarray], max_kpts: Optional[int] = None) -> device.D2NetResult:
        """Same-sized images, (H, W) gray or (H, W, 3) RGB (a fourth channel is dropped); everything stays on the
        device. Coordinates come back in the frame of the images as given, also when they were resized."""
        x = np.ascontiguousarray(np.stack(arrays), dtype=np.uint8)
        if x.ndim == 4 and x.shape[3] == 4:
            x = np.ascontiguousarray(x[..., :3])
        if x.ndim == 4 and x.shape[3] == 1:
            x = x[..., 0]
        t = torch.from_numpy(x).to(torch.device("cuda"))
        H, W = x.shape[1], x.shape[2]
        H1, W1, fact_i, fact_j = resized_shape(H, W)
        if (H1, W1) != (H, W):
            f = t.to(torch.float32)
            f = f[:, None] if f.dim() == 3 else f.permute(0, 3, 1, 2)
            f = torch.nn.functional.interpolate(f, size=(H1, W1), mode="bilinear", antialias=True, align_corners=False)
            f = f.round().clamp(0, 255).to(torch.uint8)
            t = (f[:, 0] if x.ndim == 3 else f.permute(0, 2, 3, 1)).contiguous()
        return device.d2net_extract(t, self.weights(), max_kpts or self.max_keypoints, fact_i, fact_j)

    @staticmethod
    def _unpack(res: device.D2NetResult, i: int) -> Tuple[Keypoints, np.ndarray]:
        n = int(res.count[i].item())
        xy = res.xy[i, :n].cpu().numpy()
        scores = res.scores[i, :n].cpu().numpy()
        desc = res.desc[i, :n].cpu().numpy()
        return Keypoints(coordinates=xy, responses=scores), desc

    def detect_and_describe(self, image: Image) -> Tuple[Keypoints, np.ndarray]:
        """Reference d2net.py:47-88."""
        native.require_gpu()
        return self._unpack(self.extract_batch([image.value_array]), 0)

    def detect_and_describe_batch_device(self, images: List[Image]) -> device.D2NetResult:
        """A list of same-sized images in one call; the result's tensors stay on the device."""
        native.require_gpu()
        shapes = {im.value_array.shape for im in images}
        assert len(shapes) == 1, f"detect_and_describe_batch_device takes same-sized images; got {sorted(shapes)}"
        return self.extract_batch([im.value_array for im in images])

    def detect_and_describe_batch(self, images: List[Image]) -> List[Tuple[Keypoints, np.ndarray]]:
        native.require_gpu()
        out: List[Tuple[Keypoints, np.ndarray]] = [None] * len(images)  # type: ignore
        by_shape: Dict[tuple, List[int]] = {}
        for i, im in enumerate(images):
            by_shape.setdefault(im.value_array.shape, []).append(i)
        for _, idx in by_shape.items():
            res = self.extract_batch([images[i].value_array for i in idx])
            for j, i in enumerate(idx):
                out[i] = self._unpack(res, j)
        return out
