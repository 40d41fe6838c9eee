"""Seeded random D2-Net weights and test images (test infrastructure).

The reference's checkpoint (thirdparty/d2net/weights/d2_tf.pth) is not in the tree, so parity is pinned on random
weights: tests/golden/make_d2net_golden.py loads these exact tensors into the reference's own D2Net module and records
its outputs; the tests load the same tensors into the restatement and the HIP path. He-normal scale
(std = sqrt(2 / fan_in)) keeps the activations O(1) through the ten ReLU layers, and the small biases keep about half of
every layer's units alive, so the 512-channel map is neither all zero nor saturated (tests/test_d2net_ref.py checks it).
Past the first layer every filter tap is made zero-mean over its input channels. ReLU outputs are all positive, and
plain random filters turn that common offset into a per-channel constant that grows with depth: the same channel then
wins at every location and its few local maxima are the only detections (about ten on the 11 x 15 map). Zero-mean
filters respond to the pattern only, as trained ones do, and half the locations carry a detection.
"""
import numpy as np

D2NET_LAYERS = [  # (index in dense_feature_extraction.model, cin, cout), model_test.py:16-39
    (0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256),
    (17, 256, 512), (19, 512, 512), (21, 512, 512),
]
PREFIX = "dense_feature_extraction.model"


def d2net_state_dict(seed: int = 0) -> dict:
    """{PREFIX}.{idx}.weight (cout, cin, 3, 3) float32 and .bias (cout,) float32 for every convolution."""
    rng = np.random.default_rng(seed)
    sd = {}
    for idx, cin, cout in D2NET_LAYERS:
        w = rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin))
        if cin > 3:
            w -= w.mean(axis=1, keepdims=True)
        sd[f"{PREFIX}.{idx}.weight"] = w.astype(np.float32)
        sd[f"{PREFIX}.{idx}.bias"] = rng.uniform(-0.05, 0.05, size=cout).astype(np.float32)
    return sd


def textured_image(seed: int, H: int, W: int, gray: bool = False) -> np.ndarray:
    """Textured noise, uint8 (H, W, 3) or (H, W): smooth blobs a few pixels across (a random field box-filtered
    twice) stretched to the full range, plus fine noise. The blobs survive the two poolings, so the map has distinct
    local maxima, the fine noise keeps the first layers busy."""
    rng = np.random.default_rng(seed)
    C = 1 if gray else 3
    f = rng.uniform(0.0, 1.0, (H + 8, W + 8, C))
    for _ in range(2):
        f = (f[:-2] + f[1:-1] + f[2:]) / 3.0
        f = (f[:, :-2] + f[:, 1:-1] + f[:, 2:]) / 3.0
    f = (f - f.min()) / (f.max() - f.min())
    img = 255.0 * (0.85 * f[2:2 + H, 2:2 + W] + 0.15 * rng.uniform(0.0, 1.0, (H, W, C)))
    img = np.clip(np.round(img), 0, 255).astype(np.uint8)
    return img[..., 0] if gray else img
