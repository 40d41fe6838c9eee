"""LightGlue matcher on the MI355X.

Drop-in for gtsfm/frontend/matcher/lightglue_matcher.py:24-93 (LightGlueMatcher): same constructor (features,
use_cuda), same checks (responses required -> ValueError), same output: (M, 2) uint32 (i1, i2) in ascending i1 order.
The network (d = 256, 4 heads, 9 layers of self + cross attention, adaptive depth 0.95, filter threshold 0.1) runs in
libgtsfm_hip.so (gtsfm_lightglue_batched, gtsfm_amd/csrc/lightglue.hip). Keypoint responses are required, as by the
reference wrapper, but the network does not read them.

Parity with the authors' code and with the published checkpoint is unpinned: neither is part of the reference
checkout, so the arithmetic is the one restated in DESIGN.md and tests/lightglue_ref.py. Point pruning
(width_confidence) is not built; the result is the never-pruned one.

Weights: a state dict with the upstream module's parameter names (also the older `self_attn.{i}.` / `cross_attn.{i}.`
checkpoint keys), from `weights_path` (torch.load(weights_only=True)) or passed in as `state_dict`.
"""
from pathlib import Path
from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from gtsfm_amd import device, native
from gtsfm_amd.common.keypoints import Keypoints
from gtsfm_amd.frontend.matcher.matcher_base import MatcherBase

LIGHTGLUE_DESC_DIM = 256
N_LAYERS = 9
DEPTH_CONFIDENCE = 0.95
FILTER_THRESHOLD = 0.1
WEIGHTS_PATH = Path("thirdparty/LightGlue/weights/superpoint_lightglue.pth")
_MISSING = {
    "disk": "the 128-D input_proj (Linear 128 -> 256) is not built",
    "aliked": "the 128-D input_proj (Linear 128 -> 256) is not built",
    "sift": "the scale and orientation inputs of the position encoding (and the 128-D input_proj) are not built",
    "doghardnet": "the scale and orientation inputs of the position encoding (and the 128-D input_proj) are not built",
}


def canonical_state_dict(state_dict: Dict[str, np.ndarray], n_layers: int = N_LAYERS) -> Dict[str, np.ndarray]:
    """Upstream names; older checkpoints' `self_attn.{i}.` / `cross_attn.{i}.` become `transformers.{i}.*_attn.`."""
    out = {}
    for k, v in state_dict.items():
        if k == "confidence_thresholds":
            continue
        for i in range(n_layers):
            for kind in ("self_attn", "cross_attn"):
                if k.startswith(f"{kind}.{i}."):
                    k = f"transformers.{i}.{kind}." + k[len(f"{kind}.{i}."):]
        out[k] = np.asarray(v, dtype=np.float32)
    return out


def qkv_permutation() -> np.ndarray:
    """Rows of Wqkv in the packed order [q | k | v], each head-major h * 64 + e <- upstream channel h * 192 + e * 3 + s
    (the module unflattens its 768 outputs to (heads, 64, 3))."""
    s, h, e = np.meshgrid(np.arange(3), np.arange(4), np.arange(64), indexing="ij")
    return (h * 192 + e * 3 + s).ravel()


def pack_lightglue_weights(state_dict: Dict[str, np.ndarray], n_layers: int = N_LAYERS) -> np.ndarray:
    """Upstream state dict -> the packed fp32 blob of include/gtsfm_hip.h / lightglue.hip."""
    sd = canonical_state_dict(state_dict, n_layers)
    parts = [sd["posenc.Wr.weight"].reshape(32, 2)]
    perm = qkv_permutation()

    def ffn(p):
        return [sd[f"{p}.0.weight"].T, sd[f"{p}.0.bias"], sd[f"{p}.1.weight"], sd[f"{p}.1.bias"],
                sd[f"{p}.3.weight"].T, sd[f"{p}.3.bias"]]

    for i in range(n_layers):
        s, c = f"transformers.{i}.self_attn", f"transformers.{i}.cross_attn"
        parts += [sd[f"{s}.Wqkv.weight"][perm].T, sd[f"{s}.Wqkv.bias"][perm]]
        parts += [sd[f"{s}.out_proj.weight"].T, sd[f"{s}.out_proj.bias"]] + ffn(f"{s}.ffn")
        parts += [np.concatenate([sd[f"{c}.to_qk.weight"], sd[f"{c}.to_v.weight"]], 0).T,
                  np.concatenate([sd[f"{c}.to_qk.bias"], sd[f"{c}.to_v.bias"]])]
        parts += [sd[f"{c}.to_out.weight"].T, sd[f"{c}.to_out.bias"]] + ffn(f"{c}.ffn")
        a = f"log_assignment.{i}"
        last = i + 1 == n_layers  # the last layer has no confidence head
        wt = np.zeros(256, np.float32) if last else sd[f"token_confidence.{i}.token.0.weight"].reshape(256)
        bt = np.zeros(1, np.float32) if last else sd[f"token_confidence.{i}.token.0.bias"].reshape(1)
        parts += [sd[f"{a}.final_proj.weight"].T, sd[f"{a}.final_proj.bias"], sd[f"{a}.matchability.weight"].reshape(256),
                  wt, sd[f"{a}.matchability.bias"].reshape(1), bt, np.zeros(2, np.float32)]
    return np.ascontiguousarray(np.concatenate([np.ascontiguousarray(x).ravel() for x in parts]), dtype=np.float32)


class LightGlueMatcher(MatcherBase):
    """LightGlue (SuperPoint features) computed by HIP kernels."""

    def __init__(self, features: str = "superpoint", use_cuda: bool = True,
                 state_dict: Optional[Dict[str, np.ndarray]] = None,
                 weights_path: Optional[Union[str, Path]] = None) -> None:
        super().__init__()
        if features != "superpoint":
            why = _MISSING.get(features, "only the SuperPoint variant is built")
            raise ValueError(f"LightGlueMatcher(features={features!r}) is not supported: {why}")
        self._features = features
        self._use_cuda = use_cuda
        self._state_dict = state_dict
        self._weights_path = weights_path or WEIGHTS_PATH
        self._n_layers = N_LAYERS
        self._depth_confidence = DEPTH_CONFIDENCE
        self._filter_threshold = FILTER_THRESHOLD
        self._blob: Optional[torch.Tensor] = None

    def __getstate__(self):
        s = self.__dict__.copy()
        s["_blob"] = None
        return s

    def weights(self) -> torch.Tensor:
        if self._blob is None:
            native.require_gpu()
            sd = self._state_dict
            if sd is None:
                sd = {k: v.numpy() for k, v in
                      torch.load(str(self._weights_path), map_location="cpu", weights_only=True).items()}
            self._blob = torch.from_numpy(pack_lightglue_weights(sd, self._n_layers)).to(torch.device("cuda"))
        return self._blob

    def match_batch(self, keypoints: Sequence[Keypoints], descriptors: Sequence[np.ndarray],
                    image_shapes: Sequence[Tuple[int, ...]], pairs: Sequence[Tuple[int, int]]
                    ) -> Dict[Tuple[int, int], np.ndarray]:
        """All pairs in one batched launch sequence; same per-pair output as match()."""
        n = len(keypoints)
        kmax = max([len(k) for k in keypoints] + [1])
        kmax = (kmax + 63) // 64 * 64
        kp = np.zeros((n, kmax, 2), np.float32)
        de = np.zeros((n, kmax, LIGHTGLUE_DESC_DIM), np.float32)
        cnt = np.zeros(n, np.int32)
        hw = np.zeros((n, 2), np.int32)
        for i, (k, d, s) in enumerate(zip(keypoints, descriptors, image_shapes)):
            if k.responses is None:
                raise ValueError("Responses for keypoints required for LightGlue.")
            m = len(k)
            if m and d.shape[1] != LIGHTGLUE_DESC_DIM:
                raise ValueError("LightGlue (superpoint) works on 256 dimensional descriptors")
            kp[i, :m] = k.coordinates
            de[i, :m] = d
            cnt[i] = m
            hw[i] = (s[0], s[1])
        out = {tuple(p): np.zeros((0, 2), np.uint32) for p in pairs}
        run = [p for p in pairs if cnt[p[0]] > 0 and cnt[p[1]] > 0]
        if run:
            native.require_gpu()
            dev = torch.device("cuda")
            t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
            idx, c, _, _ = device.lightglue_match(t(kp), t(de), t(cnt), t(hw),
                                                  t(np.asarray(run, np.int32).reshape(-1, 2)), self.weights(),
                                                  self._n_layers, self._depth_confidence, self._filter_threshold)
            c = c.cpu().numpy()
            w = int(c.max()) if len(c) else 0
            idx = idx[:, :w].cpu().numpy().view(np.uint32)
            for j, p in enumerate(run):
                out[tuple(p)] = idx[j, : c[j]].copy()
        return out

    def match(self, keypoints_i1: Keypoints, keypoints_i2: Keypoints, descriptors_i1: np.ndarray,
              descriptors_i2: np.ndarray, im_shape_i1: Tuple[int, int, int], im_shape_i2: Tuple[int, int, int]
              ) -> np.ndarray:
        return self.match_batch([keypoints_i1, keypoints_i2], [descriptors_i1, descriptors_i2],
                                [im_shape_i1, im_shape_i2], [(0, 1)])[(0, 1)]
