"""Seeded random PatchmatchNet weights (test infrastructure, as superpoint_weights.py is for the front-end networks).

The reference's pretrained checkpoint is not shipped, so parity is pinned on these tensors: the golden script loads them
into the reference's own PatchmatchNet and records its outputs, the tests load the same tensors into the HIP path and
into the restatement. The state dict is regenerated from the seed instead of being stored in the golden: at 175k
floats it would by itself take most of what one committed file may hold.

Kaiming-normal weights (std = sqrt(2 / fan_in)) alone give uniform scores (confidence 0.5 everywhere), so `gain`
multiplies feature.output1-3 and every conv of the three 1x1x1 nets (pixel-wise, similarity, feature weight): five
factors in a row from image to score, so the useful range of `gain` is narrow. propa_conv and eval_conv, which the
reference initialises to zero, get weights that move the sampling positions by about a pixel. BatchNorm statistics are
random: gamma U(0.5, 1.5), beta N(0, 0.1), running mean N(0, 0.1), running var U(0.5, 1.5).
"""
import numpy as np

GAIN = 1.6  # see DESIGN.md ("PatchmatchNet golden"): <= 1.5 is degenerate, >= 1.65 puts NaN into the fp32 reference

FEATURE_CONVS = [  # (name, cin, cout, kernel) of FeatureNet's ConvBnReLU layers (net.py:23-37)
    ("conv0", 3, 8, 3), ("conv1", 8, 8, 3), ("conv2", 8, 16, 5), ("conv3", 16, 16, 3), ("conv4", 16, 16, 3),
    ("conv5", 16, 32, 5), ("conv6", 32, 32, 3), ("conv7", 32, 32, 3), ("conv8", 32, 64, 5), ("conv9", 64, 64, 3),
    ("conv10", 64, 64, 3),
]
FEATURE_1X1 = [  # (name, cin, cout, bias) (net.py:39-43)
    ("output1", 64, 64, False), ("inner1", 32, 64, True), ("inner2", 16, 64, True), ("output2", 64, 32, False),
    ("output3", 64, 16, False),
]
STAGE_CHANNELS = {1: 16, 2: 32, 3: 64}
STAGE_GROUPS = {1: 4, 2: 8, 3: 8}
STAGE_PROPAGATE = {1: 0, 2: 8, 3: 16}
REFINE_CONVS = [("conv0", 3, 8), ("conv1", 1, 8), ("conv2", 8, 8), ("conv3", 16, 8)]  # net.py:87-96, all 3x3


def patchmatchnet_state_dict(seed: int = 0, gain: float = GAIN) -> dict:
    """Every tensor of PatchmatchNet().state_dict() by the reference's names, float32 (num_batches_tracked int64)."""
    rng = np.random.default_rng(seed)
    sd = {}

    def conv(name, shape, scale=1.0, bias=False, bias_std=0.05):
        fan_in = int(np.prod(shape[1:]))
        sd[f"{name}.weight"] = (rng.standard_normal(shape) * scale * np.sqrt(2.0 / fan_in)).astype(np.float32)
        if bias:
            sd[f"{name}.bias"] = (rng.standard_normal(shape[0]) * bias_std).astype(np.float32)

    def bn(name, c):
        sd[f"{name}.weight"] = rng.uniform(0.5, 1.5, size=c).astype(np.float32)
        sd[f"{name}.bias"] = (rng.standard_normal(c) * 0.1).astype(np.float32)
        sd[f"{name}.running_mean"] = (rng.standard_normal(c) * 0.1).astype(np.float32)
        sd[f"{name}.running_var"] = rng.uniform(0.5, 1.5, size=c).astype(np.float32)
        sd[f"{name}.num_batches_tracked"] = np.array(0, dtype=np.int64)

    for name, cin, cout, k in FEATURE_CONVS:
        conv(f"feature.{name}.conv", (cout, cin, k, k))
        bn(f"feature.{name}.bn", cout)
    for name, cin, cout, bias in FEATURE_1X1:
        conv(f"feature.{name}", (cout, cin, 1, 1), scale=gain if name.startswith("output") else 1.0, bias=bias)

    def mlp(name, g, last):
        conv(f"{name}.conv0.conv", (16, g, 1, 1, 1), scale=gain)
        bn(f"{name}.conv0.bn", 16)
        conv(f"{name}.conv1.conv", (8, 16, 1, 1, 1), scale=gain)
        bn(f"{name}.conv1.bn", 8)
        conv(f"{name}.{last}", (1, 8, 1, 1, 1), scale=gain, bias=True)

    for stage in (1, 2, 3):
        p, c, g = f"patchmatch_{stage}", STAGE_CHANNELS[stage], STAGE_GROUPS[stage]
        if stage == 3:
            mlp(f"{p}.evaluation.pixel_wise_net", g, "conv2")
        mlp(f"{p}.evaluation.similarity_net", g, "similarity")
        if STAGE_PROPAGATE[stage]:
            # the features carry `gain`, so the offsets are scaled back to about a pixel
            conv(f"{p}.propa_conv", (2 * STAGE_PROPAGATE[stage], c, 3, 3), scale=0.3 / gain, bias=True, bias_std=0.3)
        conv(f"{p}.eval_conv", (18, c, 3, 3), scale=0.3 / gain, bias=True, bias_std=0.3)
        mlp(f"{p}.feature_weight_net", g, "similarity")

    for name, cin, cout in REFINE_CONVS:
        conv(f"upsample_net.{name}.conv", (cout, cin, 3, 3))
        bn(f"upsample_net.{name}.bn", cout)
    conv("upsample_net.deconv", (8, 8, 3, 3))
    bn("upsample_net.bn", 8)
    conv("upsample_net.res", (1, 8, 3, 3), scale=0.2)
    return sd
