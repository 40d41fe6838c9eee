"""Seeded random LightGlue weights with the upstream module's state-dict names (a helper module, numpy only).

The magnitudes keep every stage of the network busy on unit-norm descriptors: attention logits of order one, a
feed-forward update of about a tenth of the feature's norm per block, a near-identity final projection whose gain
differs per layer (so that the assignment of a pair depends on which layer's log_assignment it uses), and Wr large
enough that rotary phases wrap.

Adaptive depth is planted. Every token-confidence head reads one unit direction G of the feature space with gain
TOKEN_GAIN, and its bias is TOKEN_BIAS[layer]. A keypoint whose descriptor carries the component alpha along G has
the token logit TOKEN_GAIN * alpha + bias (up to the feed-forward drift, a few units), so an image set whose
descriptors are given alpha = ALPHA_EARLY / ALPHA_MID / ALPHA_NEVER (lightglue_cases.make_depth_images) leaves at
layer 0, at layer LATE_LAYER, or never. Descriptors without a planted component (random component along G, token
logit of standard deviation ~ TOKEN_GAIN / 16) leave at LATE_LAYER.
"""
from typing import Dict

import numpy as np

N_LAYERS = 9
TOKEN_GAIN = 100.0
LATE_LAYER = 3
TOKEN_BIAS = [0.0 if i < LATE_LAYER else 20.0 for i in range(N_LAYERS - 1)]
ALPHA_EARLY, ALPHA_MID, ALPHA_NEVER = 0.1, -0.1, -0.4


def direction() -> np.ndarray:
    g = np.random.default_rng(7).standard_normal(256)
    return (g / np.linalg.norm(g)).astype(np.float32)


def lightglue_state_dict(seed: int = 0, n_layers: int = N_LAYERS, old_names: bool = False) -> Dict[str, np.ndarray]:
    rng = np.random.default_rng(seed)
    f = lambda *s, std=1.0: (std * rng.standard_normal(s)).astype(np.float32)  # noqa: E731
    sd = {"posenc.Wr.weight": f(32, 2, std=6.0)}
    g = direction()

    def ffn(p):
        sd[f"{p}.0.weight"], sd[f"{p}.0.bias"] = f(512, 512, std=512 ** -0.5), f(512, std=0.1)
        sd[f"{p}.1.weight"], sd[f"{p}.1.bias"] = 1.0 + f(512, std=0.1), f(512, std=0.1)
        sd[f"{p}.3.weight"], sd[f"{p}.3.bias"] = f(256, 512, std=0.01 * 512 ** -0.5), f(256, std=0.0005)

    for i in range(n_layers):
        s = f"self_attn.{i}" if old_names else f"transformers.{i}.self_attn"
        c = f"cross_attn.{i}" if old_names else f"transformers.{i}.cross_attn"
        sd[f"{s}.Wqkv.weight"], sd[f"{s}.Wqkv.bias"] = f(768, 256), f(768, std=0.1)
        sd[f"{s}.out_proj.weight"], sd[f"{s}.out_proj.bias"] = f(256, 256, std=1 / 16), f(256, std=0.1)
        ffn(f"{s}.ffn")
        sd[f"{c}.to_qk.weight"], sd[f"{c}.to_qk.bias"] = f(256, 256), f(256, std=0.1)
        sd[f"{c}.to_v.weight"], sd[f"{c}.to_v.bias"] = f(256, 256), f(256, std=0.1)
        sd[f"{c}.to_out.weight"], sd[f"{c}.to_out.bias"] = f(256, 256, std=1 / 16), f(256, std=0.1)
        ffn(f"{c}.ffn")
        a = f"log_assignment.{i}"
        gain = 12.0 + 0.5 * i  # S = gain^2 / 16 * cosine: 9 .. 16 for a true match
        sd[f"{a}.final_proj.weight"] = (gain * np.eye(256) + f(256, 256, std=0.02 * gain)).astype(np.float32)
        sd[f"{a}.final_proj.bias"] = f(256, std=0.05)
        sd[f"{a}.matchability.weight"], sd[f"{a}.matchability.bias"] = f(1, 256, std=2.0), np.float32([3.0])
        if i + 1 < n_layers:
            t = f"token_confidence.{i}.token.0"
            sd[f"{t}.weight"] = (TOKEN_GAIN * g).reshape(1, 256).astype(np.float32)
            sd[f"{t}.bias"] = np.float32([TOKEN_BIAS[i]])
    if old_names:
        sd["confidence_thresholds"] = np.zeros(n_layers, np.float32)
    return sd
