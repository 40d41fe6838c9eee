"""Planted D2-Net maps (test infrastructure): weights under which the dense map is an exactly known function of the
image, so that the trunk's indexing and the detection's handling of exact ties can be tested bit for bit.

Pass-through weights: zero biases, and in layers 0..8 a single weight of 1 from input channel c to output channel c
for c < 3 (on the centre tap unless `taps` says otherwise); in the last layer one weight gain[co] from input channel
src[co] to output channel co. Every other product is an exact zero, so no summation order can matter, and with gains
that are powers of two every product is exact. For an image made of constant 4 x 4 blocks u both max-pools pass the
block value through, and the map is

    F[co] = gain[co] * G[src[co]],   G[c] = avg2x2(relu(pre(u))[c]),

with pre the preprocessing of tests/d2net_ref.py and avg2x2 the stride-1 average pool, (((a + b) + c) + d) / 4 in raster
order. Two output channels with the same source and gain are exactly tied everywhere. tests/test_d2net_planted.py
checks the formula against the restatement's float32 map bit for bit.
"""
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

import d2net_ref as dref
from d2net_weights import D2NET_LAYERS, PREFIX

DIM = 512
TIE_CHANNELS = (0, 1, 2, 300, 301)  # gain 1; 300 copies G[0] and 301 copies G[1] (src = co % 3)
THIRD_COPY = 150                    # a third copy of G[0] for the three-way tie


def passthrough_state_dict(src: Sequence[int], gain: Sequence[float], bias: Optional[Sequence[float]] = None,
                           taps: Optional[Dict[int, Tuple[int, int]]] = None) -> Dict[str, np.ndarray]:
    """src (512,) in {0, 1, 2}, gain (512,) float32, bias: optional (512,) bias of the last layer; taps: layer number
    (0..9) -> (ky, kx), the tap that carries the layer's weights in place of the centre (1, 1). A non-centre tap
    shifts that layer's output by dilation * (k - 1) pixels, zero filled."""
    src, gain = np.asarray(src, np.int64), np.asarray(gain, np.float32)
    assert src.shape == gain.shape == (DIM,) and src.min() >= 0 and src.max() < 3
    sd = {}
    for n, (idx, cin, cout) in enumerate(D2NET_LAYERS):
        ky, kx = (taps or {}).get(n, (1, 1))
        w = np.zeros((cout, cin, 3, 3), np.float32)
        b = np.zeros(cout, np.float32)
        if n < len(D2NET_LAYERS) - 1:
            w[np.arange(3), np.arange(3), ky, kx] = 1.0
        else:
            w[np.arange(DIM), src, ky, kx] = gain
            if bias is not None:
                b[:] = np.asarray(bias, np.float32)
        sd[f"{PREFIX}.{idx}.weight"], sd[f"{PREFIX}.{idx}.bias"] = w, b
    return sd


def block_image(u: np.ndarray, extra_rows: int = 0, extra_cols: int = 0) -> np.ndarray:
    """(H4, W4, 3) uint8 -> (4 H4 + extra_rows, 4 W4 + extra_cols, 3): every value as a constant 4 x 4 block. Up to
    three extra rows and columns of 255 (the largest value there is) on the bottom and right make H and W
    non-multiples of 4; the two floor-halving max-pools must drop them, and a pool that read them would show."""
    assert u.dtype == np.uint8 and u.ndim == 3 and u.shape[2] == 3 and 0 <= extra_rows < 4 and 0 <= extra_cols < 4
    img = np.repeat(np.repeat(u, 4, axis=0), 4, axis=1)
    return np.ascontiguousarray(np.pad(img, ((0, extra_rows), (0, extra_cols), (0, 0)), constant_values=255))


def planted_source(u: np.ndarray) -> np.ndarray:
    """G (3, H4 - 1, W4 - 1) float32."""
    r = np.maximum(dref.preprocess(u), np.float32(0.0))
    assert r.dtype == np.float32
    return (((r[:, :-1, :-1] + r[:, :-1, 1:]) + r[:, 1:, :-1]) + r[:, 1:, 1:]) / np.float32(4.0)


def planted_map(u: np.ndarray, src: Sequence[int], gain: Sequence[float],
                bias: Optional[Sequence[float]] = None) -> np.ndarray:
    """The closed-form float32 map (512, H4 - 1, W4 - 1) of block_image(u) under passthrough_state_dict(src, gain)."""
    G = planted_source(u)
    F = np.asarray(gain, np.float32)[:, None, None] * G[np.asarray(src, np.int64)]
    if bias is not None:
        F = np.maximum(F + np.asarray(bias, np.float32)[:, None, None], np.float32(0.0))
    assert F.dtype == np.float32
    return F


def noise_blocks(seed: int, H4: int, W4: int) -> np.ndarray:
    """Independent uniform uint8 noise on the block grid."""
    return np.random.default_rng(seed).integers(0, 256, (H4, W4, 3), dtype=np.uint8)


def channel_sources() -> np.ndarray:
    return np.arange(DIM) % 3


def seam_gains() -> np.ndarray:
    """A distinct (source, gain) in every channel, so that a channel written to the wrong place shows. 512 distinct
    powers of two do not exist in float32; with src = co % 3 each source feeds 171 channels, and channel co gets
    2 ** (co // 3 - 85): exponents -85 .. 85. G is 0 or within [2 ** -10, 4] (the smallest positive preprocessed value
    is 0.0055), so every map value, and every product of a bf16 plane of it with a gain, is a normal float32."""
    return np.ldexp(np.float32(1.0), np.arange(DIM) // 3 - 85).astype(np.float32)


def tie_gains(three_way: bool = False) -> np.ndarray:
    """1 on TIE_CHANNELS (and on THIRD_COPY), 0.25 elsewhere: the channel maximum is always taken in the gain-1
    channels, and channels 0 / 300 (/ 150), and 1 / 301, are tied wherever they take it."""
    g = np.full(DIM, 0.25, np.float32)
    g[list(TIE_CHANNELS)] = 1.0
    if three_way:
        assert THIRD_COPY % 3 == 0
        g[THIRD_COPY] = 1.0
    return g


def tied_groups(score: np.ndarray, cij: np.ndarray):
    """Groups of candidates (indices into the candidate list, ascending) with one location and one score."""
    groups = {}
    for q, (s, (_, i, j)) in enumerate(zip(score.tolist(), cij.tolist())):
        groups.setdefault((i, j, s), []).append(q)
    return [g for g in groups.values() if len(g) > 1]


def overflow_kept(cij: np.ndarray, cap: int) -> np.ndarray:
    """Indices (ascending, so still in (c, i, j) order) of the candidates a per-image list of `cap` entries keeps: the
    first `cap` in (i, j, c) order."""
    first = np.lexsort((cij[:, 0], cij[:, 2], cij[:, 1]))[:cap]
    return np.sort(first)


def cut_between_blocks(score: np.ndarray, order: np.ndarray, groups, block: int = 256, member: int = 1):
    """A k such that rows k - 1 and k of the ranked list are members `member - 1` and `member` of one tied group and
    sit in different `block`-entry blocks of the candidate list; None if there is none."""
    row_of = np.empty(len(order), np.int64)
    row_of[order] = np.arange(len(order))
    for g in groups:
        if len(g) <= member:
            continue
        a, b = g[member - 1], g[member]
        if a // block != b // block and row_of[b] == row_of[a] + 1:
            assert score[a] == score[b]
            return int(row_of[b])
    return None


# ------------------------------------------------------------------ the cases of tests/test_d2net_edges_gpu.py
# Their preconditions are asserted without a GPU by tests/test_d2net_planted.py. The convolution's tiles are 16 rows x
# 32 columns of the map.
TIE_CASE = dict(seed=4, H4=26, W4=50)        # 104 x 200 image, 25 x 49 map
OVERFLOW_CASE = dict(seed=1, H4=18, W4=34)   # 72 x 136 image, 17 x 33 map, every gain 1
SEAM_CASES = {  # name -> (H4, W4, extra rows, extra columns)
    "16x32": (17, 33, 0, 0),   # 68 x 132: the map ends exactly on the tile edges
    "16x33": (17, 34, 3, 3),   # 71 x 139: one column past, H and W odd, H / 2 and W / 2 odd
    "17x32": (18, 33, 2, 1),   # 74 x 133: one row past, H / 2 odd
    "2x2": (3, 3, 0, 0),       # 12 x 12, the smallest legal image
}
SHIFT_GRID = (18, 34)          # 17 x 33 map: a shift crosses the tile seams and the map border
SHIFT_CASES = {  # name -> (layer, (ky, kx))
    "dilated8_tap00": (8, (0, 0)),
    "dilated8_tap22": (8, (2, 2)),
    "plain5_tap02": (5, (0, 2)),
    "pooled3_tap20": (3, (2, 0)),
}


def case_blocks(case) -> np.ndarray:
    return noise_blocks(case["seed"], case["H4"], case["W4"])


# ------------------------------------------------------------------ an edge ratio exactly on its threshold
EDGE_CHANNEL = 7


def edge_threshold_case():
    """(state dict, image, expected float32 map (512, 7, 7)) with one detection whose edge ratio tr^2 / det is exactly
    the float32 threshold 7.2f, so `<=` keeps it and `<` would not.

    Layer 1 scales the three pass-through channels by 1024 and layer 2 computes relu(1 - x): a positive preprocessed
    value (at least 0.0055) becomes 0 and a zero becomes 1, an exact indicator b_c of `u_c is dark` on the block grid.
    The last layer makes channel EDGE_CHANNEL = 10 avg2x2(b_0) + 2 avg2x2(b_1), all other channels 0. With b_0 two
    block rows and b_1 two block columns the map is P[i] + Q[j], P = (.., 0, 5, 10, 5, 0, ..), Q = (.., 0, 1, 2, 1, 0,
    ..): every value is a multiple of 1/2, so every sum is exact in any order. At the crossing (3, 3) the value is 12,
    dii = -10, djj = -2, dij = 0: det = 20, tr^2 = 144, and 144 / 20 rounds to 7.2f. Along the two ridges nothing is a
    3 x 3 maximum but their four ends at the map border, where the zero padding gives a step of exactly 0.5: a second
    exact threshold, which |step| < 0.5 rejects."""
    u = np.full((8, 8, 3), 255, np.uint8)
    u[3:5, :, 0] = 0
    u[:, 3:5, 1] = 0
    sd = passthrough_state_dict(channel_sources(), np.zeros(DIM, np.float32))
    (i1, _, _), (i2, _, _), (i9, _, _) = D2NET_LAYERS[1], D2NET_LAYERS[2], D2NET_LAYERS[9]
    for c in range(3):
        sd[f"{PREFIX}.{i1}.weight"][c, c, 1, 1] = 1024.0
        sd[f"{PREFIX}.{i2}.weight"][c, c, 1, 1] = -1.0
        sd[f"{PREFIX}.{i2}.bias"][c] = 1.0
    sd[f"{PREFIX}.{i9}.weight"][EDGE_CHANNEL, 0, 1, 1] = 10.0
    sd[f"{PREFIX}.{i9}.weight"][EDGE_CHANNEL, 1, 1, 1] = 2.0
    b = (u == 0).astype(np.float32).transpose(2, 0, 1)
    A = (((b[:, :-1, :-1] + b[:, :-1, 1:]) + b[:, 1:, :-1]) + b[:, 1:, 1:]) / np.float32(4.0)
    F = np.zeros((DIM, 7, 7), np.float32)
    F[EDGE_CHANNEL] = np.float32(10.0) * A[0] + np.float32(2.0) * A[1]
    return sd, block_image(u), F
