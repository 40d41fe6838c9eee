"""PatchmatchNet as MVSDepthFusion's depth estimator: the weight blob and the callable over gtsfm_patchmatchnet_batched.

Counterpart of the model call in gtsfm/densify/mvs_patchmatchnet.py:110-165 and of thirdparty/patchmatchnet/models
(eval mode, the reference's fixed configuration). The whole batch goes through one call: every view is a reference view
once and FeatureNet runs once per view, where the reference runs it once per (reference, source) use.
"""
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from gtsfm_amd import device, native
from gtsfm_amd.common import upload

BN_EPS = 1e-5
_FEATURE_CONVS = [f"feature.conv{i}" for i in range(11)]
_FEATURE_1X1 = ["feature.output1", "feature.inner1", "feature.inner2", "feature.output2", "feature.output3"]
_PROPAGATE = {3: True, 2: True, 1: False}


def _bn_fold(sd: Dict[str, np.ndarray], name: str) -> Tuple[np.ndarray, np.ndarray]:
    scale = sd[f"{name}.weight"] / np.sqrt(sd[f"{name}.running_var"] + BN_EPS)
    return scale, sd[f"{name}.bias"] - sd[f"{name}.running_mean"] * scale


def _conv(weight: np.ndarray, bias: Optional[np.ndarray], scale: Optional[np.ndarray] = None,
          shift: Optional[np.ndarray] = None) -> np.ndarray:
    """weight (co, ci, k, k) -> W[ky][kx][ci][co] then bias[co], with an optional per-output scale and shift."""
    co = weight.shape[0]
    b = np.zeros(co) if bias is None else bias.astype(np.float64)
    w = weight.astype(np.float64)
    if scale is not None:
        w, b = w * scale[:, None, None, None], b * scale + shift
    return np.concatenate((w.transpose(2, 3, 1, 0).ravel(), b))


def _mlp(sd: Dict[str, np.ndarray], name: str, last: str) -> np.ndarray:
    """A 1x1x1 net: W0[G][16], b0[16], W1[16][8], b1[8], W2[8], b2[1], BatchNorm folded."""
    out = []
    for i in (0, 1):
        scale, shift = _bn_fold(sd, f"{name}.conv{i}.bn")
        w = sd[f"{name}.conv{i}.conv.weight"].astype(np.float64).reshape(scale.size, -1) * scale[:, None]
        out += [w.T.ravel(), shift]
    out += [sd[f"{name}.{last}.weight"].astype(np.float64).ravel(), sd[f"{name}.{last}.bias"].astype(np.float64)]
    return np.concatenate(out)


def pack_patchmatchnet_weights(state_dict) -> np.ndarray:
    """The fp32 blob gtsfm_patchmatchnet_batched reads (layout: include/gtsfm_hip.h) from PatchmatchNet's state dict,
    tensors or arrays; the `module.` prefix of the reference's nn.DataParallel checkpoint is accepted. BatchNorm is
    folded in fp64 and rounded once."""
    sd = {}
    for k, v in state_dict.items():
        k = k[len("module."):] if k.startswith("module.") else k
        sd[k] = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    sd = {k: v.astype(np.float64) for k, v in sd.items() if not k.endswith("num_batches_tracked")}

    def cbr(name):
        return _conv(sd[f"{name}.conv.weight"], None, *_bn_fold(sd, f"{name}.bn"))

    parts = [cbr(name) for name in _FEATURE_CONVS]
    parts += [_conv(sd[f"{name}.weight"], sd.get(f"{name}.bias")) for name in _FEATURE_1X1]
    for stage in (3, 2, 1):
        p = f"patchmatch_{stage}"
        if stage == 3:
            parts.append(_mlp(sd, f"{p}.evaluation.pixel_wise_net", "conv2"))
        parts.append(_mlp(sd, f"{p}.evaluation.similarity_net", "similarity"))
        if _PROPAGATE[stage]:
            parts.append(_conv(sd[f"{p}.propa_conv.weight"], sd[f"{p}.propa_conv.bias"]))
        parts.append(_conv(sd[f"{p}.eval_conv.weight"], sd[f"{p}.eval_conv.bias"]))
        parts.append(_mlp(sd, f"{p}.feature_weight_net", "similarity"))
    u = "upsample_net"
    parts += [cbr(f"{u}.conv0"), cbr(f"{u}.conv1"), cbr(f"{u}.conv2")]
    # ConvTranspose2d's weight is (ci, co, k, k): swap to (co, ci, k, k) for _conv; the kernel indexes taps directly
    parts.append(_conv(sd[f"{u}.deconv.weight"].transpose(1, 0, 2, 3), None, *_bn_fold(sd, f"{u}.bn")))
    parts += [cbr(f"{u}.conv3"), _conv(sd[f"{u}.res.weight"], None)]
    return np.concatenate(parts).astype(np.float32)


class PatchmatchNetDepthEstimator:
    """`depth_estimator(images, proj_inputs, depth_range) -> (depth, confidence)` for MVSDepthFusion, on the HIP
    PatchmatchNet. weights: a state dict, or the packed blob as an array or device tensor. The random initialisation's
    uniform numbers come from a device generator seeded with `seed` at every call, so a call can be repeated."""

    def __init__(self, weights, seed: int = 0) -> None:
        self._blob = weights if isinstance(weights, (np.ndarray, torch.Tensor)) else pack_patchmatchnet_weights(weights)
        self._seed = int(seed)

    def init_uniform(self, n: int, H: int, W: int, dev: torch.device) -> torch.Tensor:
        gen = torch.Generator(device=dev)
        gen.manual_seed(self._seed)
        return torch.rand((n, native.PATCHMATCHNET_INIT_BINS, H // 8, W // 8), dtype=torch.float32, device=dev,
                          generator=gen)

    def __call__(self, images: torch.Tensor, proj_inputs, depth_range: torch.Tensor
                 ) -> Tuple[torch.Tensor, torch.Tensor]:
        wRc, wtc, intrinsics, src_views = proj_inputs
        n, H, W = images.shape[:3]
        dev = images.device
        if n == 0 or src_views.shape[1] == 0:
            raise ValueError("PatchmatchNet needs at least one source view per reference view")
        if not isinstance(self._blob, torch.Tensor) or self._blob.device != dev:
            self._blob = upload.to_device(np.ascontiguousarray(self._blob, np.float32), dev) \
                if isinstance(self._blob, np.ndarray) else self._blob.to(dev)
        r = device.patchmatchnet_depth(images.contiguous(), wRc.contiguous(), wtc.contiguous(),
                                       intrinsics.contiguous(), src_views.contiguous(),
                                       depth_range.to(torch.float64).contiguous(), self._blob,
                                       self.init_uniform(n, H, W, dev))
        return r.depth, r.confidence
