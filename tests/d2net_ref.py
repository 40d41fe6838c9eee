"""Torch restatement of the D2-Net single-scale path that gtsfm_d2net_batched computes (include/gtsfm_hip.h), written
from that description and run in a chosen dtype: the fp64 run is the tests' truth, the fp32 run the yardstick for what
fp32 arithmetic costs. tests/test_d2net_ref.py pins it against outputs recorded from the reference's own modules.
"""
from typing import Dict

import numpy as np
import torch
import torch.nn.functional as F

from d2net_weights import D2NET_LAYERS, PREFIX

MEAN = np.array([0.485, 0.456, 0.406])
STD = np.array([0.229, 0.224, 0.225])
EDGE_LIMIT = (5 + 1) ** 2 / 5


def to_rgb(image: np.ndarray) -> np.ndarray:
    image = np.asarray(image)
    return np.repeat(image[:, :, None], 3, axis=2) if image.ndim == 2 else image


def preprocess(image: np.ndarray) -> np.ndarray:
    """uint8 (H, W, 3) -> float32 (3, H, W): / 255 in float32, then normalised in float64 and narrowed."""
    x = to_rgb(image).astype(np.float32).transpose(2, 0, 1) / np.float32(255.0)
    return ((x.astype(np.float64) - MEAN[:, None, None]) / STD[:, None, None]).astype(np.float32)


def dense_map(sd, image: np.ndarray, dtype: torch.dtype, device="cpu") -> torch.Tensor:
    """(512, h, w) map of the trunk. sd: name -> array, or tensors already on `device` in `dtype`."""
    x = torch.from_numpy(preprocess(image))[None].to(device, dtype)
    for n, (idx, _, _) in enumerate(D2NET_LAYERS):
        w = torch.as_tensor(sd[f"{PREFIX}.{idx}.weight"]).to(device, dtype)
        b = torch.as_tensor(sd[f"{PREFIX}.{idx}.bias"]).to(device, dtype)
        d = 2 if n >= 7 else 1
        x = F.relu(F.conv2d(x, w, b, padding=d, dilation=d))
        if n in (1, 3):
            x = F.max_pool2d(x, 2, 2)
        if n == 6:
            x = F.avg_pool2d(x, 2, 1)
    return x[0]


def _shift(Fp: torch.Tensor, di: int, dj: int) -> torch.Tensor:
    h, w = Fp.shape[1] - 2, Fp.shape[2] - 2
    return Fp[:, 1 + di:1 + di + h, 1 + dj:1 + dj + w]


def fields(Fm: torch.Tensor) -> Dict[str, torch.Tensor]:
    """Every per-element quantity of the detection and the localisation, each (512, h, w)."""
    Fp = F.pad(Fm, (1, 1, 1, 1))
    up, down, left, right = _shift(Fp, -1, 0), _shift(Fp, 1, 0), _shift(Fp, 0, -1), _shift(Fp, 0, 1)
    dii = up - 2 * Fm + down
    djj = left - 2 * Fm + right
    dij = 0.25 * (_shift(Fp, -1, -1) - _shift(Fp, -1, 1) - _shift(Fp, 1, -1) + _shift(Fp, 1, 1))
    det = dii * djj - dij * dij
    tr = dii + djj
    di, dj = 0.5 * (down - up), 0.5 * (right - left)
    step_i = -((djj / det) * di + (-dij / det) * dj)
    step_j = -((-dij / det) * di + (dii / det) * dj)
    cmax = Fm.max(dim=0, keepdim=True)[0]
    # the largest in-map 3x3 neighbour, the centre left out
    Fn = F.pad(Fm, (1, 1, 1, 1), value=float("-inf"))
    nmax = torch.stack([_shift(Fn, a, b) for a in (-1, 0, 1) for b in (-1, 0, 1) if (a, b) != (0, 0)]).max(0)[0]
    # the largest other channel at the location
    top2 = Fm.topk(2, dim=0)[0]
    other = torch.where(Fm == top2[0:1], top2[1:2], top2[0:1])
    return dict(dii=dii, djj=djj, dij=dij, det=det, tr=tr, ratio=tr * tr / det, step_i=step_i, step_j=step_j,
                cmax=cmax.expand_as(Fm), nmax=nmax, other=other)


def detect(Fm: torch.Tensor) -> Dict[str, np.ndarray]:
    """Candidates in (c, i, j) order with their positions, and how many detections each later test rejected."""
    q = fields(Fm)
    h, w = Fm.shape[1:]
    is_max = (Fm == q["cmax"]) & (Fm >= q["nmax"])
    not_edge = (q["det"] > 0) & (q["ratio"] <= EDGE_LIMIT)
    detected = is_max & not_edge
    idx = torch.nonzero(detected)  # lexicographic (c, i, j)
    c, i, j = idx[:, 0], idx[:, 1], idx[:, 2]
    si, sj = q["step_i"][c, i, j], q["step_j"][c, i, j]
    near = (si.abs() < 0.5) & (sj.abs() < 0.5)
    pi, pj = i.to(Fm.dtype) + si, j.to(Fm.dtype) + sj
    inside = (pi.floor() >= 0) & (pi.ceil() < h) & (pj.floor() >= 0) & (pj.ceil() < w)
    keep = near & inside
    # maxima of a positive value only: an all-zero location ties every channel at 0 but its det is 0
    return dict(cij=idx[keep].cpu().numpy(), pi=pi[keep].cpu().numpy(), pj=pj[keep].cpu().numpy(),
                score=Fm[c, i, j][keep].cpu().numpy(),
                rejected_edge=int((is_max & (Fm > 0) & ~not_edge).sum()), rejected_step=int((~near).sum()),
                rejected_corner=int((near & ~inside).sum()))


def describe(Fm: torch.Tensor, pi: np.ndarray, pj: np.ndarray) -> np.ndarray:
    pi, pj = torch.from_numpy(pi).to(Fm.device, Fm.dtype), torch.from_numpy(pj).to(Fm.device, Fm.dtype)
    i0, j0, i1, j1 = pi.floor().long(), pj.floor().long(), pi.ceil().long(), pj.ceil().long()
    a, b = pi - i0.to(Fm.dtype), pj - j0.to(Fm.dtype)
    d = ((1 - a) * (1 - b) * Fm[:, i0, j0] + (1 - a) * b * Fm[:, i0, j1] + a * (1 - b) * Fm[:, i1, j0]
         + a * b * Fm[:, i1, j1])
    d = d / d.norm(dim=0, keepdim=True).clamp_min(1e-12)
    return d.t().contiguous().cpu().numpy()


def run(sd, image: np.ndarray, dtype: torch.dtype, max_keypoints: int = 5000, fact_i: float = 1.0,
        fact_j: float = 1.0, device="cpu") -> Dict[str, np.ndarray]:
    """dense (512, h, w); candidates cij (N, 3) in list order with cand_pos (N, 2) = (p_i, p_j), cand_score, cand_desc
    (N, 512); and the final keypoints: order (indices into the candidate list, descending score, ties by position), xy
    (K, 2) = (x, y), scores (K,), desc (K, 512)."""
    with torch.no_grad():
        Fm = dense_map(sd, image, dtype, device)
        det = detect(Fm)
        desc = describe(Fm, det["pi"], det["pj"])
    order = np.argsort(-det["score"], kind="stable")[:max_keypoints]
    up = np.stack([det["pj"], det["pi"]], axis=1)
    for _ in range(2):
        up = up * 2 + 0.5
    up = up * np.array([fact_j, fact_i], up.dtype)
    out = dict(dense=Fm.cpu().numpy(), cij=det["cij"], cand_pos=np.stack([det["pi"], det["pj"]], axis=1),
               cand_score=det["score"], cand_desc=desc, order=order, xy=up[order], scores=det["score"][order],
               desc=desc[order])
    out.update({k: det[k] for k in ("rejected_edge", "rejected_step", "rejected_corner")})
    return out


def margins(Fm64: np.ndarray) -> Dict[str, np.ndarray]:
    """For every element of the fp64 map, the distance of each test from its threshold, in the units the slack of
    tests/test_d2net_gpu.py is given in (map units; the edge ratio and the step are pure numbers, and are scaled by the
    map's maximum so that one slack serves). An element is `decided` for a slack s when no test can flip under a map
    perturbation of that order: every margin's absolute value is above s, or an earlier test already fails by more
    than s. `detected` is the restatement's decision."""
    Fm = torch.from_numpy(Fm64)
    q = fields(Fm)
    h, w = Fm.shape[1:]
    scale = float(Fm.max())
    ii = torch.arange(h, dtype=Fm.dtype)[None, :, None].expand_as(Fm)
    jj = torch.arange(w, dtype=Fm.dtype)[None, None, :].expand_as(Fm)
    pi, pj = ii + q["step_i"], jj + q["step_j"]
    # corner test: with |step| < 0.5 it fails only at the border rows / columns, by the sign of the step
    corner = torch.full_like(Fm, float("inf"))
    corner = torch.where(ii == 0, torch.minimum(corner, q["step_i"] * scale), corner)
    corner = torch.where(ii == h - 1, torch.minimum(corner, -q["step_i"] * scale), corner)
    corner = torch.where(jj == 0, torch.minimum(corner, q["step_j"] * scale), corner)
    corner = torch.where(jj == w - 1, torch.minimum(corner, -q["step_j"] * scale), corner)
    m = dict(channel=Fm - q["other"], local=Fm - q["nmax"], det=q["det"] / scale,
             edge=(EDGE_LIMIT - q["ratio"]) * scale,
             step=(0.5 - torch.maximum(q["step_i"].abs(), q["step_j"].abs())) * scale, corner=corner)
    inside = (pi.floor() >= 0) & (pi.ceil() < h) & (pj.floor() >= 0) & (pj.ceil() < w)
    detected = ((Fm == q["cmax"]) & (Fm >= q["nmax"]) & (q["det"] > 0) & (q["ratio"] <= EDGE_LIMIT)
                & (q["step_i"].abs() < 0.5) & (q["step_j"].abs() < 0.5) & inside)
    out = {k: torch.nan_to_num(v, nan=0.0).numpy() for k, v in m.items()}
    out["detected"] = detected.numpy()
    return out


def map_error(dense: np.ndarray, dense64: np.ndarray):
    """(median, 99th percentile, max) of |dense - dense64| relative to the fp64 map's maximum."""
    e = np.abs(dense.astype(np.float64) - dense64) / dense64.max()
    return float(np.median(e)), float(np.percentile(e, 99)), float(e.max())


def slack_for(dense32: np.ndarray, dense64: np.ndarray) -> float:
    """The keypoint comparison's slack, in map units: 100 x the fp32 restatement's map error. Half of the map is
    exactly 0 after the last ReLU in either precision, so the median error is 0 and the 99th percentile is the
    measured error that is used."""
    return 100.0 * map_error(dense32, dense64)[1] * float(dense64.max())


def compare_detected(m: Dict[str, np.ndarray], slack: float, got_cij: np.ndarray):
    """got_cij (N, 3): a detected set to hold against the fp64 decision where fp32 cannot flip it. Returns (missing,
    spurious, dropped share): decided detections that `got` lacks, elements of `got` that are decidedly none, and the
    share of undecided elements (candidates and near-candidates) relative to the number of candidates."""
    sure_in, sure_out = decided(m, slack)
    got = np.zeros_like(sure_in)
    got[got_cij[:, 0], got_cij[:, 1], got_cij[:, 2]] = True
    missing = np.argwhere(sure_in & ~got)
    spurious = np.argwhere(sure_out & got)
    dropped = float((~(sure_in | sure_out)).sum()) / max(int(m["detected"].sum()), 1)
    assert not (sure_in & ~m["detected"]).any() and not (sure_out & m["detected"]).any()
    return missing, spurious, dropped


def decided(m: Dict[str, np.ndarray], slack: float):
    """(surely detected, surely not detected) for a map perturbation of order `slack`: an element is surely detected
    when every margin exceeds the slack, surely rejected when some margin is below -slack; the rest are near a
    threshold and are left out of the comparison."""
    names = ("channel", "local", "det", "edge", "step", "corner")
    sure_in = np.logical_and.reduce([m[k] > slack for k in names])
    sure_out = np.logical_or.reduce([m[k] < -slack for k in names])
    return sure_in, sure_out
