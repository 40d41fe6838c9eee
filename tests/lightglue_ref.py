"""The LightGlue network at SuperPoint's width restated in torch, with the dtype as a parameter (a helper module).

This is the oracle of tests/test_lightglue_ref.py and tests/test_lightglue_gpu.py: the arithmetic of DESIGN.md's
LightGlue section, written from that specification and not from the kernels. The authors' source and checkpoint are
not available to the tests, so parity with them is unpinned; what is pinned is that the kernels compute this.
State-dict names are the upstream module's.
"""
import math
from typing import Dict, NamedTuple, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

HEADS, HD, D = 4, 64, 256


class Result(NamedTuple):
    matches: np.ndarray     # (M, 2) int64, ascending first index
    matches0: np.ndarray    # (n0,) int64, -1 = none
    mscores0: np.ndarray    # (n0,)
    Z: np.ndarray           # (n0 + 1, n1 + 1) log-assignment with the dustbin column / row
    exit_layer: int
    decisions: list         # per confidence layer run: (below, near, total, stopped): `near` counts confidences
    #                         within 1e-3 of the threshold


def threshold(layer: int, n_layers: int = 9) -> float:
    return float(np.clip(0.8 + 0.1 * math.exp(-4.0 * layer / n_layers), 0.0, 1.0))


def _rot(t):
    a, b = t.unflatten(-1, (-1, 2)).unbind(-1)
    return torch.stack((-b, a), -1).flatten(-2)


def _ffn(W, p, x, m):
    h = torch.cat([x, m], -1) @ W[f"{p}.0.weight"].T + W[f"{p}.0.bias"]
    h = F.layer_norm(h, (2 * D,), W[f"{p}.1.weight"], W[f"{p}.1.bias"], eps=1e-5)
    return F.gelu(h) @ W[f"{p}.3.weight"].T + W[f"{p}.3.bias"]


def _heads(t):  # (n, 256) with channel h * 64 + e -> (heads, n, 64)
    return t.unflatten(-1, (HEADS, HD)).transpose(0, 1)


def lightglue(kp0, kp1, desc0, desc1, hw0: Tuple[int, int], hw1: Tuple[int, int], sd: Dict[str, np.ndarray],
              dtype=torch.float64, depth_confidence: float = 0.95, filter_threshold: float = 0.1, n_layers: int = 9,
              rotary: bool = True, assign_layer: Optional[int] = None, device=None) -> Result:
    """One pair. rotary=False removes the rotary step; assign_layer overrides which layer's log_assignment weights the
    assignment uses (the tests show that the wrong layer's weights give another answer). device: where torch
    computes (tools/lightglue_bench.py times the restatement on the GPU); `sd` may hold tensors already there."""
    def T(v):
        return torch.as_tensor(v if isinstance(v, torch.Tensor) else np.asarray(v), dtype=dtype, device=device)

    W = {k: T(v) for k, v in sd.items()}
    n0, n1 = len(kp0), len(kp1)
    if n0 == 0 or n1 == 0:
        return Result(np.zeros((0, 2), np.int64), np.full(n0, -1, np.int64), np.zeros(n0), np.zeros((0, 0)),
                      n_layers - 1, [])

    def encode(kp, hw):
        Hi, Wi = hw
        size = T([Wi, Hi])
        p = (T(kp) - size / 2) / (max(Wi, Hi) / 2)
        th = p @ W["posenc.Wr.weight"].T  # (n, 32)
        return th.cos().repeat_interleave(2, -1), th.sin().repeat_interleave(2, -1)

    enc = [encode(kp0, hw0), encode(kp1, hw1)]
    x = [T(desc0), T(desc1)]
    exit_layer, decisions = n_layers - 1, []
    for i in range(n_layers):
        p = f"transformers.{i}.self_attn"
        for s in range(2):
            qkv = (x[s] @ W[f"{p}.Wqkv.weight"].T + W[f"{p}.Wqkv.bias"]).unflatten(-1, (HEADS, HD, 3))
            q, k, v = (qkv[..., j].transpose(0, 1) for j in range(3))  # (heads, n, 64)
            if rotary:
                c, sn = enc[s]
                q, k = q * c + _rot(q) * sn, k * c + _rot(k) * sn
            ctx = torch.softmax(q @ k.transpose(-1, -2) / 8, -1) @ v
            msg = ctx.transpose(0, 1).flatten(-2) @ W[f"{p}.out_proj.weight"].T + W[f"{p}.out_proj.bias"]
            x[s] = x[s] + _ffn(W, f"{p}.ffn", x[s], msg)
        p = f"transformers.{i}.cross_attn"
        qk = [_heads(t @ W[f"{p}.to_qk.weight"].T + W[f"{p}.to_qk.bias"]) for t in x]
        vv = [_heads(t @ W[f"{p}.to_v.weight"].T + W[f"{p}.to_v.bias"]) for t in x]
        sim = qk[0] @ qk[1].transpose(-1, -2) / 8
        m = [torch.softmax(sim, -1) @ vv[1], torch.softmax(sim.transpose(-1, -2), -1) @ vv[0]]
        m = [t.transpose(0, 1).flatten(-2) @ W[f"{p}.to_out.weight"].T + W[f"{p}.to_out.bias"] for t in m]
        x = [x[s] + _ffn(W, f"{p}.ffn", x[s], m[s]) for s in range(2)]
        if i + 1 < n_layers and depth_confidence > 0:
            t = f"token_confidence.{i}.token.0"
            conf = torch.cat([torch.sigmoid(xs @ W[f"{t}.weight"].T + W[f"{t}.bias"]).flatten() for xs in x])
            tau = threshold(i, n_layers)
            below = int((conf < tau).sum())
            near = int(((conf - tau).abs() < 1e-3).sum())
            stop = 1.0 - below / (n0 + n1) > depth_confidence
            decisions.append((below, near, n0 + n1, bool(stop)))
            if stop:
                exit_layer = i
                break
    a = f"log_assignment.{exit_layer if assign_layer is None else assign_layer}"
    md = [(t @ W[f"{a}.final_proj.weight"].T + W[f"{a}.final_proj.bias"]) / D ** 0.25 for t in x]
    S = md[0] @ md[1].T
    z = [(t @ W[f"{a}.matchability.weight"].T + W[f"{a}.matchability.bias"]).flatten() for t in x]
    Z = torch.zeros((n0 + 1, n1 + 1), dtype=dtype, device=device)
    Z[:n0, :n1] = (F.log_softmax(S, 1) + F.log_softmax(S, 0) + F.logsigmoid(z[0])[:, None]
                   + F.logsigmoid(z[1])[None, :])
    Z[:n0, n1] = F.logsigmoid(-z[0])
    Z[n0, :n1] = F.logsigmoid(-z[1])
    Zn = Z.cpu().numpy()
    matches, matches0, mscores0 = matches_of(Zn, filter_threshold)
    return Result(matches, matches0, mscores0, Zn, exit_layer, decisions)


def matches_of(Z: np.ndarray, filter_threshold: float = 0.1):
    """Mutual row / column argmax over the interior (lowest index on ties), kept where exp(Z) > threshold."""
    core = Z[:-1, :-1]
    n0 = core.shape[0]
    m0, m1 = core.argmax(1), core.argmax(0)
    mutual = m1[m0] == np.arange(n0)
    ms = np.where(mutual, np.exp(core[np.arange(n0), m0]), 0.0)
    valid = mutual & (ms > filter_threshold)
    matches0 = np.where(valid, m0, -1).astype(np.int64)
    i = np.flatnonzero(valid)
    return np.stack([i, m0[i]], 1).astype(np.int64), matches0, ms
