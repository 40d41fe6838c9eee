"""Device-resident batched entry points over the C ABI (include/gtsfm_hip.h).

torch provides HBM allocations and the stream; every computation is a libgtsfm_hip.so kernel. Tensors passed
in must already live on the GPU; nothing here copies to the host or synchronises (except the measurement hook
match_pairs(stats=...)).
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from gtsfm_amd import native

_F32, _F64, _I32, _I64, _U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _u64(seed: int) -> int:
    return int(seed) & (2 ** 64 - 1)


def _flag(b) -> int:
    return 1 if b else 0


def _check(t: Optional[torch.Tensor], name: str, dtype: Union[torch.dtype, Tuple[torch.dtype, ...]],
           numel: Optional[int] = None, shape: Optional[Sequence[Optional[int]]] = None,
           min_numel: Optional[int] = None, optional: bool = False) -> None:
    """Every wrapper's tensor check: `t` is a contiguous device tensor of `dtype` (one, or a tuple to choose from)
    with `numel` elements (or at least `min_numel`) or of `shape` (None = any extent); None passes when `optional`.
    Raises AssertionError naming the argument."""
    if t is None and optional:
        return
    ok = t is not None and t.is_cuda and t.is_contiguous() and \
        (t.dtype in dtype if isinstance(dtype, tuple) else t.dtype == dtype)
    if ok and numel is not None:
        ok = t.numel() == numel
    if ok and min_numel is not None:
        ok = t.numel() >= min_numel
    if ok and shape is not None:
        ok = t.dim() == len(shape) and all(s is None or s == d for s, d in zip(shape, t.shape))
    if not ok:
        want = "".join(f", {k} {v}" for k, v in (("numel", numel), ("numel >=", min_numel), ("shape", shape))
                       if v is not None)
        got = "None" if t is None else f"{t.dtype} {tuple(t.shape)} on {t.device}, strides {t.stride()}"
        raise AssertionError(f"{name} must be a contiguous device tensor of {dtype}{want}; got {got}")


def _check_cameras(wRc: torch.Tensor, wtc: torch.Tensor, intrinsics: torch.Tensor,
                   cam_valid: Optional[torch.Tensor]) -> int:
    """Checks per-image poses (wRc, wtc), intrinsics (f, u0, v0) and the optional valid bytes; returns n_img."""
    n_img = intrinsics.numel() // 3
    _check(wRc, "wRc", _F64, numel=9 * n_img)
    _check(wtc, "wtc", _F64, numel=3 * n_img)
    _check(intrinsics, "intrinsics", _F64, numel=3 * n_img)
    _check(cam_valid, "cam_valid", _U8, numel=n_img, optional=True)
    return n_img


def _track_csr(track_offsets: Optional[torch.Tensor], track_img: Optional[torch.Tensor],
               track_uv: Optional[torch.Tensor], n_tracks: Optional[int],
               n_tracks_dev: Optional[torch.Tensor]) -> Tuple[int, int, int]:
    """Checks a track CSR (track_offsets (>= T + 1,) int32, track_img (n_meas,) int32, track_uv (n_meas, 2) float32 or
    float64, n_tracks_dev int64 or None) and returns (T, n_meas, uv_is_f64). T is n_tracks, or track_offsets.numel()
    - 1 (0 for an empty track_offsets); no CSR at all (track_offsets None) is (0, 0, 0)."""
    _check(n_tracks_dev, "n_tracks_dev", _I64, min_numel=1, optional=True)
    if track_offsets is None:
        return 0, 0, 0
    _check(track_offsets, "track_offsets", _I32)
    _check(track_img, "track_img", _I32)
    n_meas = track_img.numel()
    _check(track_uv, "track_uv", (_F32, _F64), numel=2 * n_meas)
    T = max(track_offsets.numel() - 1, 0) if n_tracks is None else int(n_tracks)
    assert 0 <= T <= max(track_offsets.numel() - 1, 0), f"n_tracks {T} for {track_offsets.numel()} track_offsets"
    return T, n_meas, _flag(track_uv.dtype == _F64)


def _workspace(nbytes: int, device: torch.device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def _take_workspace(need: int, device: torch.device, workspace: Optional[torch.Tensor],
                    stream: Optional[torch.cuda.Stream], unsupported: Optional[str] = None) -> torch.Tensor:
    """The workspace tensor to hand to the library: the caller's if it holds `need` bytes, else a fresh one (never
    below 256 bytes), recorded on `stream` since the kernels may still read it after the wrapper returns. need == 0
    is the library's word for a shape it does not take: with `unsupported` given it raises that as NativeError."""
    if need == 0 and unsupported is not None:
        raise native.NativeError(unsupported)
    ws = workspace if workspace is not None and workspace.numel() >= need else _workspace(need, device)
    if stream is not None:
        ws.record_stream(stream)
    return ws


def match_pairs(desc: torch.Tensor, counts: torch.Tensor, pairs: torch.Tensor, ratio: Optional[float],
                mode: int = native.GTSFM_MATCH_INT_F16, stream: Optional[torch.cuda.Stream] = None,
                groups: Optional[torch.Tensor] = None,
                out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                stats: Optional[dict] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Mutual-NN + ratio matching of every (i1, i2) row of `pairs`.

    Args:
        desc: (n_img, kmax, dim) float32 descriptors on the GPU (rows >= counts[i] are ignored).
        counts: (n_img,) int32 valid rows per image.
        pairs: (P, 2) int32 image index pairs.
        ratio: ratio-test threshold, or None for plain mutual NN.
        mode: GTSFM_MATCH_INT_F16 (integer descriptors, MFMA) or GTSFM_MATCH_EXACT_F32.
        groups: optional (n_groups, G) int32 device tensor of pair indices (-1 = empty slot) for the INT_F16 kernel:
            every pair exactly once, the pairs of a group sharing image i1 (pair_groups builds one).
        out: optional caller-owned (idx (P, kmax, 2) int32, count (P,) int32) to write into (no allocation: a
            pipelined caller keeps them across steps instead of cycling cross-stream blocks through the allocator).
        stats: optional dict filled, for GTSFM_MATCH_F16_RERANK with dim <= 512, with the certificate's counts
            (gtsfm_match_rerank_stats; synchronises the stream): "keypoint_sides" (sum over pairs of both images'
            counts), "uncertified" and "uncertified_frac" (entries the fp16 shortlist did not certify, recomputed
            exactly), "tiled_frac" (entries of (pair, side)s recomputed whole by the exact tile kernel) and
            "rescan_frac" (uncertified entries rescanned one keypoint at a time).

    Returns:
        idx: (P, kmax, 2) int32 tensor holding uint32 keypoint indices, rows [0, count) valid per pair.
        count: (P,) int32.
    """
    _check(desc, "desc", _F32, shape=(None, None, None))
    _check(counts, "counts", _I32)
    _check(pairs, "pairs", _I32)
    n_img, kmax, dim = desc.shape
    n_pairs = pairs.shape[0]
    L = native.lib()
    if out is not None:
        idx, cnt = out
        _check(idx, "out[0]", _I32, shape=(n_pairs, kmax, 2))
        _check(cnt, "out[1]", _I32, shape=(n_pairs,))
        cnt.zero_()
    else:
        idx = torch.empty((max(n_pairs, 1), kmax, 2), dtype=torch.int32, device=desc.device)
        cnt = torch.zeros((max(n_pairs, 1),), dtype=torch.int32, device=desc.device)
    if n_pairs == 0:
        return idx[:0], cnt[:0]
    _check(groups, "groups", _I32, shape=(None, None), optional=True)
    ws = _take_workspace(L.gtsfm_match_workspace_bytes(n_img, kmax, dim, n_pairs, mode), desc.device, None, stream)
    rc = L.gtsfm_match_batched_grouped(
        _ptr(desc), _ptr(counts), n_img, kmax, dim, _ptr(pairs), n_pairs,
        _ptr(groups), 0 if groups is None else groups.shape[0],
        0 if groups is None else groups.shape[1], -1.0 if ratio is None else float(ratio), mode, _ptr(ws),
        ws.numel(), _ptr(idx), _ptr(cnt), native.stream_handle(stream))
    native.check(rc, "gtsfm_match_batched_grouped")
    if stats is not None and mode == native.GTSFM_MATCH_F16_RERANK and dim <= native.GTSFM_MATCH_F16_MAX_DIM:
        unc = np.zeros(2 * n_pairs, dtype=np.int32)
        n_unc = ctypes.c_int(0)
        native.check(L.gtsfm_match_rerank_stats(_ptr(ws), ws.numel(), n_img, kmax, dim, n_pairs, ctypes.byref(n_unc),
                                                unc.ctypes.data, native.stream_handle(stream)),
                     "gtsfm_match_rerank_stats")
        c = counts.cpu().numpy().astype(np.int64)
        pr = pairs.cpu().numpy().astype(np.int64)
        nq = np.concatenate([c[pr[:, 0]], c[pr[:, 1]]])  # side 0: rows of i1, side 1: rows of i2
        tiled = (unc > 0) & (unc.astype(np.int64) * 32 >= nq)
        total = max(int(nq.sum()), 1)
        stats.update(keypoint_sides=int(nq.sum()), uncertified=int(n_unc.value),
                     uncertified_frac=int(n_unc.value) / total, tiled_frac=int(nq[tiled].sum()) / total,
                     rescan_frac=int(unc[~tiled].sum()) / total)
    return idx, cnt


def match_group_size(kmax: int, dim: int) -> int:
    """Largest pairs-per-workgroup the INT_F16 distance GEMM holds for this kmax / dim (0: not supported)."""
    return int(native.lib().gtsfm_match_max_group(int(kmax), int(dim)))


def _split_cost(n_groups: int, group_size: int, kmax: int, n_cu: int) -> float:
    """Estimated time (in pair-passes of one workgroup) of a grouped distance-GEMM launch, with the pass split the
    library picks for it (matcher.hip pp_split: n_split in {1, 2, 4} minimising ceil(n_groups * n_split / CUs) *
    (passes / n_split))."""
    npass = -(-kmax // 512)
    best = None
    s = 1
    while s <= 4 and s <= npass:
        t = -(-(n_groups * s) // n_cu) * -(-npass // s)
        best = t if best is None or t < best else best
        s *= 2
    return float(best) * group_size


def match_plan(pairs: np.ndarray, kmax: int, dim: int, n_cu: Optional[int] = None) -> Optional[np.ndarray]:
    """Pair groups for the INT_F16 distance GEMM (gtsfm_match_batched_grouped), sized to fill the GPU: the largest
    group size (most reuse of the register operand) is kept unless a smaller one, together with the library's pass
    split, finishes in fewer estimated workgroup rounds. A rank's share of C2 at 8 GPUs (~619 pairs dealt in whole
    (i1, i2 // 4) runs, sharding.rank_pairs) has ~160 groups of 4 for 256 CUs: full groups of 2 split over pass ranges
    take 10 pair-passes of time instead of 12."""
    gmax = match_group_size(kmax, dim)
    if gmax <= 1:
        return None
    if n_cu is None:
        n_cu = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count \
            if torch.cuda.is_available() else 256
    plans = [(g, pair_groups(pairs, g)) for g in range(gmax, 0, -1)]
    cost = [_split_cost(len(groups), g, kmax, n_cu) for g, groups in plans]
    # the estimate ignores what a smaller group loses (the register operand re-read per pair, more workgroups):
    # a smaller group must win by more than 10 %
    best = min(cost)
    return next(groups for (g, groups), t in zip(plans, cost) if t <= 1.1 * best)


def pair_groups(pairs: np.ndarray, group_size: int) -> np.ndarray:
    """Tile an (P, 2) pair list into groups for the INT_F16 distance GEMM: each group = up to `group_size` pairs
    (i1, i2) sharing i1 (the register operand) with i2 in one block of `group_size` consecutive image ids, ordered
    block-major, so the ~32 workgroups resident on one XCD stream the same few i2 images from its L2 while each reads
    its own i1 once. Returns (n_groups, group_size) int32 pair indices, -1 for empty slots."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    P = len(pairs)
    if P == 0 or group_size <= 1:
        return np.arange(P, dtype=np.int32).reshape(-1, 1)
    blk = pairs[:, 1] // group_size
    order = np.lexsort((pairs[:, 1], pairs[:, 0], blk))  # block-major, then i1, then i2
    key = blk[order] * (int(pairs[:, 0].max()) + 1) + pairs[order, 0]
    starts = np.flatnonzero(np.r_[True, key[1:] != key[:-1]])
    sizes = np.diff(np.r_[starts, P])
    rank = np.arange(P) - np.repeat(starts, sizes)           # position inside its (block, i1) run
    n_sub = -(-sizes // group_size)                           # groups per run (> 1 only for repeated pairs)
    first = np.r_[0, np.cumsum(n_sub)[:-1]]
    gid = np.repeat(first, sizes) + rank // group_size
    out = np.full((int(n_sub.sum()), group_size), -1, dtype=np.int32)
    out[gid, rank % group_size] = order
    return out


@dataclass(eq=False)
class RansacResult:
    """Per-pair verifier outputs (device tensors): E, R (i2Ri1), t (i2ti1), n_inliers, status, n_hyp, mask, and
    n_models (candidate models scored; E path only, else None)."""

    E: torch.Tensor
    R: torch.Tensor
    t: torch.Tensor
    n_inliers: torch.Tensor
    status: torch.Tensor
    n_hyp: torch.Tensor
    mask: torch.Tensor
    n_models: Optional[torch.Tensor] = None


def _check_two_view(kp_xy: torch.Tensor, intrinsics: torch.Tensor, pairs: torch.Tensor, match_idx: torch.Tensor,
                    match_count: torch.Tensor, pair_ids: Optional[torch.Tensor]) -> None:
    """The verifiers' inputs: kp_xy (n_img, kmax, 2) float32, intrinsics float64, match_idx / match_count int32 and
    the optional (P,) int32 sampler keys."""
    _check(kp_xy, "kp_xy", _F32, shape=(None, None, None))
    _check(intrinsics, "intrinsics", _F64)
    _check(match_idx, "match_idx", _I32)
    _check(match_count, "match_count", _I32)
    _check(pair_ids, "pair_ids", _I32, numel=pairs.shape[0], optional=True)


def ransac_essential(kp_xy: torch.Tensor, intrinsics: torch.Tensor, pairs: torch.Tensor, match_idx: torch.Tensor,
                     match_count: torch.Tensor, thr_px: float, prob: float = 0.999999, max_iters: int = 1000,
                     seed: int = native.RANSAC_DEFAULT_SEED, pair_id_base: int = 0,
                     pair_ids: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None,
                     scoring: int = native.GTSFM_RANSAC_SCORING_MSAC) -> RansacResult:
    """Batched 5-point RANSAC + LO + recoverPose for every pair (gtsfm_ransac_E_batched).
    scoring: GTSFM_RANSAC_SCORING_MSAC (USAC_ACCURATE, the reference's default) or _RANSAC (inlier count).

    Args:
        kp_xy: (n_img, kmax, 2) float32 keypoint pixels; intrinsics: (n_img, 3) float64 (f, u0, v0).
        pairs: (P, 2) int32; match_idx: (P, mcap, 2) int32 (uint32 values); match_count: (P,) int32.
        pair_ids: optional (P,) int32 sampler keys (default pair_id_base + p).
    """
    _check_two_view(kp_xy, intrinsics, pairs, match_idx, match_count, pair_ids)
    n_img, kmax, _ = kp_xy.shape
    P = pairs.shape[0]
    mcap = match_idx.shape[1]
    dev = kp_xy.device
    L = native.lib()
    # outputs carved from two zeroed buffers (one fill each instead of one per output; pairs the verifier rejects keep
    # zero E / R / t, as do the mask entries past a pair's match count)
    P1 = max(P, 1)
    f64 = torch.zeros(21 * P1, dtype=torch.float64, device=dev)
    E, R, t = f64[:9 * P1].view(P1, 3, 3), f64[9 * P1:18 * P1].view(P1, 3, 3), f64[18 * P1:].view(P1, 3)
    i32 = torch.zeros(4 * P1, dtype=torch.int32, device=dev)
    n_inl, status, n_hyp, n_models = (i32[j * P1:(j + 1) * P1] for j in range(4))
    mask = torch.zeros((P1, max(mcap, 1)), dtype=torch.uint8, device=dev)
    if P > 0:
        ws = _take_workspace(L.gtsfm_ransac_workspace_bytes(P, mcap), dev, None, stream)
        rc = L.gtsfm_ransac_E_batched(_ptr(kp_xy), _ptr(intrinsics), n_img, kmax, _ptr(pairs), P, _ptr(match_idx),
                                      _ptr(match_count), mcap, float(thr_px), float(prob), int(max_iters), int(scoring),
                                      int(seed),
                                      int(pair_id_base), _ptr(pair_ids), _ptr(ws), ws.numel(), _ptr(E), _ptr(R), _ptr(t),
                                      _ptr(n_inl), _ptr(status), _ptr(n_hyp), _ptr(n_models), _ptr(mask),
                                      native.stream_handle(stream))
        native.check(rc, "gtsfm_ransac_E_batched")
    return RansacResult(E[:P], R[:P], t[:P], n_inl[:P], status[:P], n_hyp[:P], mask[:P], n_models[:P])


def compact_verified(match_idx: torch.Tensor, match_count: torch.Tensor, res: "RansacResult", min_inliers: int,
                     min_inlier_ratio: float, capacity: int, out_offsets: Optional[torch.Tensor] = None,
                     out_v_corr: Optional[torch.Tensor] = None, out_isp_ok: Optional[torch.Tensor] = None,
                     stream: Optional[torch.cuda.Stream] = None, ratio_inliers: Optional[torch.Tensor] = None
                     ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Inlier rows of every pair, concatenated in pair order, + the inlier-support verdict (gtsfm_compact_verified).
    `res` supplies mask / status / n_inliers (a RansacResult, or a BA2Result for the post-BA rows); ratio_inliers
    optionally gives the counts the inlier ratio is taken on (the pre-BA ones after BA).

    Returns offsets (P + 1,) int32, v_corr (capacity, 2) int32 holding uint32 indices (rows offsets[p] ..
    offsets[p + 1] belong to pair p, matcher order), isp_ok (P,) uint8.
    """
    _check(match_idx, "match_idx", _I32, shape=(None, None, None))
    P, mcap = match_idx.shape[0], match_idx.shape[1]
    _check(res.mask, "res.mask", _U8, shape=(P, mcap if P else None))
    dev = match_idx.device
    offsets = out_offsets if out_offsets is not None else torch.empty(P + 1, dtype=torch.int32, device=dev)
    v_corr = out_v_corr if out_v_corr is not None else torch.empty((max(capacity, 1), 2), dtype=torch.int32, device=dev)
    isp_ok = out_isp_ok if out_isp_ok is not None else torch.empty(max(P, 1), dtype=torch.uint8, device=dev)
    assert offsets.numel() >= P + 1 and v_corr.shape[0] >= capacity and isp_ok.numel() >= P
    rc = native.lib().gtsfm_compact_verified(_ptr(match_idx), _ptr(match_count), mcap, _ptr(res.mask),
                                             _ptr(res.status), _ptr(res.n_inliers), _ptr(ratio_inliers), P,
                                             int(min_inliers),
                                             float(min_inlier_ratio), _ptr(offsets), _ptr(v_corr), int(capacity),
                                             _ptr(isp_ok), native.stream_handle(stream))
    native.check(rc, "gtsfm_compact_verified")
    return offsets, v_corr, isp_ok


@dataclass(eq=False)
class BA2Result:
    """Post-BA per-pair outputs (device tensors): R (i2Ri1), t (unit i2ti1), mask (P, mcap) over the putatives,
    n_inliers (its row count), ba_status (0 ok, 1 no track, 2 none valid, 3 not run), iters, and `status` = the
    verifier's status (what the reference's R is None / not None follows)."""

    R: torch.Tensor
    t: torch.Tensor
    mask: torch.Tensor
    n_inliers: torch.Tensor
    ba_status: torch.Tensor
    iters: torch.Tensor
    status: torch.Tensor


def bundle_adjust_2view(kp_xy: torch.Tensor, intrinsics: torch.Tensor, pairs: torch.Tensor, match_idx: torch.Tensor,
                        match_count: torch.Tensor, res: "RansacResult", min_inliers: int = 15, max_iters: int = 100,
                        reproj_thresh: float = 0.5, tri_thresh: float = 100.0,
                        stream: Optional[torch.cuda.Stream] = None, prior_Rt: Optional[torch.Tensor] = None,
                        prior_sigmas: Optional[torch.Tensor] = None) -> BA2Result:
    """Two-view triangulation + bundle adjustment of every verified pair (gtsfm_ba2_batched) on the verifier's
    outputs `res` (same tensors as ransac_essential took). prior_Rt (P, 12) float64 (i2Ti1 R row-major, t) and
    prior_sigmas (P, 6) float64: optional relative-pose priors (a row with sigma[0] <= 0 has none)."""
    _check(kp_xy, "kp_xy", _F32)
    _check(intrinsics, "intrinsics", _F64)
    _check(match_idx, "match_idx", _I32)
    n_img, kmax = kp_xy.shape[0], kp_xy.shape[1]
    P, mcap = match_idx.shape[0], match_idx.shape[1]
    assert (prior_Rt is None) == (prior_sigmas is None), "prior_Rt and prior_sigmas come together"
    _check(prior_Rt, "prior_Rt", _F64, shape=(P, 12), optional=True)
    _check(prior_sigmas, "prior_sigmas", _F64, shape=(P, 6), optional=True)
    dev = kp_xy.device
    L = native.lib()
    R = torch.zeros((max(P, 1), 3, 3), dtype=torch.float64, device=dev)
    t = torch.zeros((max(P, 1), 3), dtype=torch.float64, device=dev)
    mask = torch.zeros((max(P, 1), max(mcap, 1)), dtype=torch.uint8, device=dev)
    n_out = torch.zeros(max(P, 1), dtype=torch.int32, device=dev)
    st = torch.zeros_like(n_out)
    iters = torch.zeros_like(n_out)
    if P > 0:
        ws = _take_workspace(L.gtsfm_ba2_workspace_bytes(P, mcap), dev, None, stream)
        rc = L.gtsfm_ba2_batched(_ptr(kp_xy), _ptr(intrinsics), n_img, kmax, _ptr(pairs), P, _ptr(match_idx),
                                 _ptr(match_count), mcap, _ptr(res.mask), _ptr(res.R.contiguous()),
                                 _ptr(res.t.contiguous()), _ptr(res.status), _ptr(prior_Rt), _ptr(prior_sigmas),
                                 int(min_inliers), int(max_iters),
                                 float(reproj_thresh), float(tri_thresh), _ptr(ws), ws.numel(), _ptr(R), _ptr(t),
                                 _ptr(mask), _ptr(n_out), _ptr(st), _ptr(iters), native.stream_handle(stream))
        native.check(rc, "gtsfm_ba2_batched")
    return BA2Result(R[:P], t[:P], mask[:P], n_out[:P], st[:P], iters[:P], res.status)


def sampson_sq(F: torch.Tensor, row_pair: torch.Tensor, x1: torch.Tensor, x2: torch.Tensor,
               precision: int = native.GTSFM_SAMPSON_F64, stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """Squared Sampson distance of row r = (x1[r], x2[r]) under F[row_pair[r]] (gtsfm_sampson_sq_batched).

    F: (n_mats, 3, 3) float64; row_pair: (N,) int32; x1, x2: (N, 2) float64. Returns (N,) float64.
    """
    _check(F, "F", _F64)
    _check(x1, "x1", _F64)
    _check(x2, "x2", _F64)
    assert x1.shape[0] == x2.shape[0], "x1 and x2 have one row each per measurement"
    _check(row_pair, "row_pair", _I32, numel=x1.shape[0])
    out = torch.empty(max(x1.shape[0], 1), dtype=torch.float64, device=F.device)
    rc = native.lib().gtsfm_sampson_sq_batched(_ptr(F), F.shape[0], _ptr(row_pair), _ptr(x1), _ptr(x2), x1.shape[0],
                                               int(precision), _ptr(out), native.stream_handle(stream))
    native.check(rc, "gtsfm_sampson_sq_batched")
    return out[: x1.shape[0]]


class FundamentalResult(RansacResult):
    """Per-pair F-path outputs: F plus everything RansacResult holds (E = K2^T F K1)."""

    def __init__(self, F, E, R, t, n_inliers, status, n_hyp, mask):
        super().__init__(E, R, t, n_inliers, status, n_hyp, mask)
        self.F = F


def ransac_fundamental(kp_xy: torch.Tensor, intrinsics: torch.Tensor, pairs: torch.Tensor, match_idx: torch.Tensor,
                       match_count: torch.Tensor, thr_px: float, prob: float = 0.999999, max_iters: int = 1000000,
                       seed: int = native.RANSAC_DEFAULT_SEED, pair_id_base: int = 0,
                       pair_ids: Optional[torch.Tensor] = None,
                       stream: Optional[torch.cuda.Stream] = None) -> FundamentalResult:
    """Batched 7-point RANSAC / LMedS F estimation + 8-point refit + E + recoverPose (gtsfm_ransac_F_batched).

    Same tensor conventions as ransac_essential; thr_px is in pixels (no focal-length scaling).
    """
    _check_two_view(kp_xy, intrinsics, pairs, match_idx, match_count, pair_ids)
    n_img, kmax, _ = kp_xy.shape
    P = pairs.shape[0]
    mcap = match_idx.shape[1]
    dev = kp_xy.device
    L = native.lib()
    F = torch.zeros((max(P, 1), 3, 3), dtype=torch.float64, device=dev)
    E, R = torch.zeros_like(F), torch.zeros_like(F)
    t = torch.zeros((max(P, 1), 3), dtype=torch.float64, device=dev)
    n_inl = torch.zeros((max(P, 1),), dtype=torch.int32, device=dev)
    status, n_hyp = torch.zeros_like(n_inl), torch.zeros_like(n_inl)
    mask = torch.zeros((max(P, 1), max(mcap, 1)), dtype=torch.uint8, device=dev)
    if P > 0:
        ws = _take_workspace(L.gtsfm_ransac_F_workspace_bytes(P, mcap), dev, None, stream)
        rc = L.gtsfm_ransac_F_batched(_ptr(kp_xy), _ptr(intrinsics), n_img, kmax, _ptr(pairs), P, _ptr(match_idx),
                                      _ptr(match_count), mcap, float(thr_px), float(prob), int(max_iters), int(seed),
                                      int(pair_id_base), _ptr(pair_ids), _ptr(ws), ws.numel(), _ptr(F), _ptr(E),
                                      _ptr(R), _ptr(t), _ptr(n_inl), _ptr(status), _ptr(n_hyp), _ptr(mask),
                                      native.stream_handle(stream))
        native.check(rc, "gtsfm_ransac_F_batched")
    return FundamentalResult(F[:P], E[:P], R[:P], t[:P], n_inl[:P], status[:P], n_hyp[:P], mask[:P])


@dataclass(eq=False)
class SiftResult:
    """Per-image SIFT outputs (device tensors): xy (n,k,2), attr (n,k,3) size/angle/response, desc (n,k,128),
    count (n,), n_detected (n,)."""

    xy: torch.Tensor
    attr: torch.Tensor
    desc: torch.Tensor
    count: torch.Tensor
    n_detected: torch.Tensor


def sift_extract(images: torch.Tensor, max_kpts: int, stream: Optional[torch.cuda.Stream] = None,
                 out: Optional[SiftResult] = None, workspace: Optional[torch.Tensor] = None,
                 masks: Optional[torch.Tensor] = None) -> SiftResult:
    """SIFT + top-k on a batch of same-sized uint8 images (n, H, W) gray or (n, H, W, 3) RGB (gtsfm_sift_batched).
    masks: optional (n, H, W) uint8; keypoints on zero pixels are dropped before the top-k."""
    _check(images, "images", _U8)
    _check(masks, "masks", _U8, shape=tuple(images.shape[:3]), optional=True)
    n = images.shape[0]
    H, W = images.shape[1], images.shape[2]
    C = 1 if images.dim() == 3 else images.shape[3]
    dev = images.device
    L = native.lib()
    if out is None:
        out = SiftResult(torch.empty((n, max_kpts, 2), dtype=torch.float32, device=dev),
                         torch.empty((n, max_kpts, 3), dtype=torch.float32, device=dev),
                         torch.empty((n, max_kpts, 128), dtype=torch.float32, device=dev),
                         torch.empty((n,), dtype=torch.int32, device=dev),
                         torch.empty((n,), dtype=torch.int32, device=dev))
    ws = _take_workspace(L.gtsfm_sift_workspace_bytes(n, H, W, max_kpts), dev, workspace, stream)
    rc = L.gtsfm_sift_batched(_ptr(images), _ptr(masks), n, H, W, C, max_kpts, _ptr(ws), ws.numel(), _ptr(out.xy),
                              _ptr(out.attr),
                              _ptr(out.desc), _ptr(out.count), _ptr(out.n_detected), native.stream_handle(stream))
    native.check(rc, "gtsfm_sift_batched")
    return out


@dataclass(eq=False)
class SuperPointResult:
    """Per-image SuperPoint outputs (device tensors): xy (n,k,2) float32 (x, y), scores (n,k), desc (n,k,256),
    count (n,), n_detected (n,)."""

    xy: torch.Tensor
    scores: torch.Tensor
    desc: torch.Tensor
    count: torch.Tensor
    n_detected: torch.Tensor


def superpoint_extract(images: torch.Tensor, weights: torch.Tensor, max_kpts: int, keypoint_threshold: float = 0.005,
                       nms_radius: int = 4, remove_borders: int = 4,
                       stream: Optional[torch.cuda.Stream] = None, out: Optional[SuperPointResult] = None,
                       workspace: Optional[torch.Tensor] = None, masks: Optional[torch.Tensor] = None
                       ) -> SuperPointResult:
    """SuperPoint on a batch of same-sized uint8 images (n, H, W) gray or (n, H, W, 3) RGB (gtsfm_superpoint_batched).

    weights: the packed fp32 blob (gtsfm_amd.frontend.detector_descriptor.superpoint.pack_superpoint_weights).
    out: optional preallocated outputs (xy (n,k,2), scores (n,k), desc (n,k,256), count, n_detected; rows past a
    count are unspecified); workspace: optional device buffer of at least gtsfm_superpoint_workspace_bytes.
    masks: optional (n, H, W) uint8 device tensor; a detection at (x, y) is kept iff masks[i, y, x] == 1 (the
    reference's Keypoints.filter_by_mask), before the top-k.
    """
    _check(images, "images", _U8)
    L = native.lib()
    _check(weights, "weights", _F32, numel=L.gtsfm_superpoint_weights_floats())
    n, H, W = images.shape[0], images.shape[1], images.shape[2]
    C = 1 if images.dim() == 3 else images.shape[3]
    dev = images.device
    if out is None:
        out = SuperPointResult(torch.zeros((n, max_kpts, 2), dtype=torch.float32, device=dev),
                               torch.zeros((n, max_kpts), dtype=torch.float32, device=dev),
                               torch.empty((n, max_kpts, 256), dtype=torch.float32, device=dev),
                               torch.zeros((n,), dtype=torch.int32, device=dev),
                               torch.zeros((n,), dtype=torch.int32, device=dev))
    _check(out.xy, "out.xy", _F32, shape=(n, max_kpts, 2))
    _check(out.scores, "out.scores", _F32, shape=(n, max_kpts))
    _check(out.desc, "out.desc", _F32, shape=(n, max_kpts, 256))
    if n == 0:
        return out
    _check(masks, "masks", _U8, shape=(n, H, W), optional=True)
    ws = _take_workspace(L.gtsfm_superpoint_workspace_bytes(n, H, W, max_kpts), dev, workspace, stream)
    rc = L.gtsfm_superpoint_batched(_ptr(images), _ptr(masks), n, H, W, C,
                                    _ptr(weights), max_kpts, float(keypoint_threshold),
                                    int(nms_radius), int(remove_borders), _ptr(ws), ws.numel(), _ptr(out.xy),
                                    _ptr(out.scores), _ptr(out.desc), _ptr(out.count), _ptr(out.n_detected),
                                    native.stream_handle(stream))
    native.check(rc, "gtsfm_superpoint_batched")
    return out


@dataclass(eq=False)
class D2NetResult:
    """Per-image D2-Net outputs (device tensors): xy (n,k,2) float32 (x, y), scores (n,k) descending, desc (n,k,512)
    unit-norm, count (n,), n_candidates (n,) (detections before the top-k); rows past a count are zero. dense_map
    (n,h,w,512) only when asked for."""

    xy: torch.Tensor
    scores: torch.Tensor
    desc: torch.Tensor
    count: torch.Tensor
    n_candidates: torch.Tensor
    dense_map: Optional[torch.Tensor] = None


def d2net_map_shape(H: int, W: int) -> Tuple[int, int]:
    """(h, w) of D2-Net's dense map for an H x W image: two floor-halvings, then the 2x2 stride-1 average pool."""
    return H // 2 // 2 - 1, W // 2 // 2 - 1


def d2net_extract(images: torch.Tensor, weights: torch.Tensor, max_kpts: int, fact_i: float = 1.0,
                  fact_j: float = 1.0, stream: Optional[torch.cuda.Stream] = None, out: Optional[D2NetResult] = None,
                  workspace: Optional[torch.Tensor] = None, dense_map: bool = False,
                  last_stage: Optional[int] = None) -> D2NetResult:
    """D2-Net (single scale) on a batch of same-sized uint8 images (n, H, W, 3) RGB or (n, H, W) gray
    (gtsfm_d2net_batched).

    weights: the packed fp32 blob (gtsfm_amd.frontend.detector_descriptor.d2net.pack_d2net_weights).
    fact_i, fact_j: row / column factors the coordinates are multiplied by (original over resized shape).
    out: optional preallocated outputs; workspace: optional device buffer of at least gtsfm_d2net_workspace_bytes.
    dense_map: also return the (n, h, w, 512) feature map (tests). last_stage: stop after that
    native.GTSFM_D2NET_STAGE_* (gtsfm_d2net_stages, the benchmark's hook); None runs the whole call.
    """
    _check(images, "images", _U8)
    L = native.lib()
    _check(weights, "weights", _F32, numel=L.gtsfm_d2net_weights_floats())
    assert images.dim() in (3, 4), f"images must be (n, H, W) or (n, H, W, 3); got {tuple(images.shape)}"
    n, H, W = images.shape[0], images.shape[1], images.shape[2]
    C = 1 if images.dim() == 3 else images.shape[3]
    dev = images.device
    if out is None:
        out = D2NetResult(torch.zeros((n, max_kpts, 2), dtype=torch.float32, device=dev),
                          torch.zeros((n, max_kpts), dtype=torch.float32, device=dev),
                          torch.zeros((n, max_kpts, 512), dtype=torch.float32, device=dev),
                          torch.zeros((n,), dtype=torch.int32, device=dev),
                          torch.zeros((n,), dtype=torch.int32, device=dev))
    _check(out.xy, "out.xy", _F32, shape=(n, max_kpts, 2))
    _check(out.scores, "out.scores", _F32, shape=(n, max_kpts))
    _check(out.desc, "out.desc", _F32, shape=(n, max_kpts, 512))
    _check(out.count, "out.count", _I32, numel=n)
    _check(out.n_candidates, "out.n_candidates", _I32, numel=n)
    if n == 0:
        return out
    need = L.gtsfm_d2net_workspace_bytes(n, H, W, max_kpts)
    ws = _take_workspace(need, dev, workspace, stream,
                         unsupported=f"gtsfm_d2net_batched takes no {n} x {H} x {W} batch with max_keypoints {max_kpts}")
    if dense_map and out.dense_map is None:
        h, w = d2net_map_shape(H, W)
        out.dense_map = torch.zeros((n, h, w, 512), dtype=torch.float32, device=dev)
    args = (_ptr(images), n, H, W, C, _ptr(weights), max_kpts, float(fact_i), float(fact_j), _ptr(ws), ws.numel(),
            _ptr(out.xy), _ptr(out.scores), _ptr(out.desc), _ptr(out.count), _ptr(out.n_candidates),
            _ptr(out.dense_map) if dense_map else None)
    if last_stage is None:
        rc = L.gtsfm_d2net_batched(*args, native.stream_handle(stream))
    else:
        rc = L.gtsfm_d2net_stages(*args, int(last_stage), native.stream_handle(stream))
    native.check(rc, "gtsfm_d2net_batched")
    return out


def superglue_match(kp: torch.Tensor, scores: torch.Tensor, desc: torch.Tensor, counts: torch.Tensor,
                    image_hw: torch.Tensor, pairs: torch.Tensor, weights: torch.Tensor, n_layers: int = 18,
                    sinkhorn_iters: int = 20, match_threshold: float = 0.2,
                    stream: Optional[torch.cuda.Stream] = None, workspace: Optional[torch.Tensor] = None
                    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """SuperGlue over every pair (gtsfm_superglue_batched).

    Args: kp (n_img, kmax, 2) f32, scores (n_img, kmax) f32, desc (n_img, kmax, 256) f32, counts (n_img,) int32,
    image_hw (n_img, 2) int32 (H, W), pairs (P, 2) int32, weights: the packed blob. kmax must be a multiple of 64.
    Returns idx (P, kmax, 2) int32 (uint32 values, i ascending), count (P,) int32, mscores0 (P, kmax) f32.
    """
    _check(kp, "kp", _F32)
    n_img, kmax = kp.shape[0], kp.shape[1]
    assert kmax % 64 == 0, f"kmax {kmax} is no multiple of 64"
    _check(scores, "scores", _F32, shape=(n_img, kmax))
    _check(desc, "desc", _F32, shape=(n_img, kmax, 256))
    for t, name in ((counts, "counts"), (image_hw, "image_hw"), (pairs, "pairs")):
        _check(t, name, _I32)
    L = native.lib()
    _check(weights, "weights", _F32, numel=L.gtsfm_superglue_weights_floats(n_layers))
    P = pairs.shape[0]
    dev = kp.device
    idx = torch.zeros((max(P, 1), kmax, 2), dtype=torch.int32, device=dev)
    cnt = torch.zeros((max(P, 1),), dtype=torch.int32, device=dev)
    ms = torch.zeros((max(P, 1), kmax), dtype=torch.float32, device=dev)
    if P > 0:
        ws = _take_workspace(L.gtsfm_superglue_workspace_bytes(P, kmax), dev, workspace, stream)
        rc = L.gtsfm_superglue_batched(_ptr(kp), _ptr(scores), _ptr(desc), _ptr(counts), _ptr(image_hw), n_img, kmax,
                                       _ptr(pairs), P, _ptr(weights), int(n_layers), int(sinkhorn_iters),
                                       float(match_threshold), _ptr(ws), ws.numel(), _ptr(idx), _ptr(cnt), _ptr(ms),
                                       native.stream_handle(stream))
        native.check(rc, "gtsfm_superglue_batched")
    return idx[:P], cnt[:P], ms[:P]


def superglue_log_assignment(workspace: torch.Tensor, n_pairs: int, kmax: int, pair: int,
                             stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """Pair `pair`'s final log-assignment matrix (kmax + 1, kmax + 1) from the workspace of the superglue_match call
    that used `workspace` (gtsfm_superglue_log_assignment; entries past (m + 1, n + 1) are NaN)."""
    out = torch.empty((kmax + 1, kmax + 1), dtype=torch.float32, device=workspace.device)
    rc = native.lib().gtsfm_superglue_log_assignment(_ptr(workspace), workspace.numel(), n_pairs, kmax, pair, _ptr(out),
                                                     native.stream_handle(stream))
    native.check(rc, "gtsfm_superglue_log_assignment")
    return out


def lightglue_match(kp: torch.Tensor, desc: torch.Tensor, counts: torch.Tensor, image_hw: torch.Tensor,
                    pairs: torch.Tensor, weights: torch.Tensor, n_layers: int = 9, depth_confidence: float = 0.95,
                    filter_threshold: float = 0.1, stream: Optional[torch.cuda.Stream] = None,
                    workspace: Optional[torch.Tensor] = None
                    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """LightGlue over every pair (gtsfm_lightglue_batched).

    Args: kp (n_img, kmax, 2) f32, desc (n_img, kmax, 256) f32, counts (n_img,) int32, image_hw (n_img, 2) int32
    (H, W), pairs (P, 2) int32, weights: the packed blob. kmax must be a multiple of 64. depth_confidence <= 0
    disables adaptive depth.
    Returns idx (P, kmax, 2) int32 (uint32 values, i ascending), count (P,) int32, mscores0 (P, kmax) f32 and
    exit_layer (P,) int32.
    """
    _check(kp, "kp", _F32)
    n_img, kmax = kp.shape[0], kp.shape[1]
    assert kmax % 64 == 0, f"kmax {kmax} is no multiple of 64"
    _check(desc, "desc", _F32, shape=(n_img, kmax, 256))
    for t, name in ((counts, "counts"), (image_hw, "image_hw"), (pairs, "pairs")):
        _check(t, name, _I32)
    L = native.lib()
    _check(weights, "weights", _F32, numel=L.gtsfm_lightglue_weights_floats(n_layers))
    P = pairs.shape[0]
    dev = kp.device
    idx = torch.zeros((max(P, 1), kmax, 2), dtype=torch.int32, device=dev)
    cnt = torch.zeros((max(P, 1),), dtype=torch.int32, device=dev)
    ms = torch.zeros((max(P, 1), kmax), dtype=torch.float32, device=dev)
    ex = torch.zeros((max(P, 1),), dtype=torch.int32, device=dev)
    if P > 0:
        ws = _take_workspace(L.gtsfm_lightglue_workspace_bytes(P, kmax), dev, workspace, stream)
        rc = L.gtsfm_lightglue_batched(_ptr(kp), _ptr(desc), _ptr(counts), _ptr(image_hw), n_img, kmax, _ptr(pairs), P,
                                       _ptr(weights), int(n_layers), float(depth_confidence), float(filter_threshold),
                                       _ptr(ws), ws.numel(), _ptr(idx), _ptr(cnt), _ptr(ms), _ptr(ex),
                                       native.stream_handle(stream))
        native.check(rc, "gtsfm_lightglue_batched")
    return idx[:P], cnt[:P], ms[:P], ex[:P]


def lightglue_log_assignment(workspace: torch.Tensor, n_pairs: int, kmax: int, pair: int,
                             stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """Pair `pair`'s log-assignment matrix (kmax + 1, kmax + 1) from the workspace of the lightglue_match call that
    used `workspace` (gtsfm_lightglue_log_assignment; entries past (m + 1, n + 1) are NaN)."""
    out = torch.empty((kmax + 1, kmax + 1), dtype=torch.float32, device=workspace.device)
    rc = native.lib().gtsfm_lightglue_log_assignment(_ptr(workspace), workspace.numel(), n_pairs, kmax, pair, _ptr(out),
                                                     native.stream_handle(stream))
    native.check(rc, "gtsfm_lightglue_log_assignment")
    return out


def retrieval_similarity(desc: torch.Tensor, blocksize: int,
                         stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """(N, N) f32 block-upper-triangular similarity of N global descriptors (N, D) f32 on the device
    (gtsfm_retrieval_similarity; netvlad_retriever.py:77-149)."""
    if desc.dim() != 2 or desc.dtype != torch.float32 or not desc.is_cuda:
        raise ValueError("desc must be a (N, D) float32 device tensor")
    desc = desc.contiguous()
    n, d = desc.shape
    sim = torch.empty((n, n), dtype=torch.float32, device=desc.device)
    if n == 0:
        return sim
    native.check(native.lib().gtsfm_retrieval_similarity(_ptr(desc), n, d, int(blocksize), _ptr(sim),
                                                         native.stream_handle(stream)),
                 "gtsfm_retrieval_similarity")
    return sim


def retrieval_pairs(scores: torch.Tensor, num_select: int, min_score: Optional[float],
                    invalid: Optional[torch.Tensor] = None,
                    stream: Optional[torch.cuda.Stream] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Top-k valid pairs per row of a (K1, K2) f32 device score matrix (gtsfm_retrieval_pairs;
    netvlad_retriever.py:196-228). invalid: (K1, K2) bool device mask, None = every entry not strictly above the
    diagonal (:164-167). Returns (pairs (K1, k, 2) int32, row_count (K1,) int32): row i's first row_count[i] entries
    are its finite top-k pairs in rank order."""
    if scores.dim() != 2 or scores.dtype != torch.float32 or not scores.is_cuda:
        raise ValueError("scores must be a (K1, K2) float32 device tensor")
    if num_select < 0:
        raise ValueError("num_select must be >= 0")
    scores = scores.contiguous()
    n1, n2 = scores.shape
    k = min(int(num_select), n1)
    if k > n2:
        raise RuntimeError(f"selected index k={k} out of range for {n2} columns")  # torch.topk's error
    inv = None
    if invalid is not None:
        if tuple(invalid.shape) != (n1, n2):
            raise ValueError("invalid must have the shape of scores")
        inv = invalid.to(device=scores.device, dtype=torch.uint8).contiguous()
    out = torch.empty((n1, k, 2), dtype=torch.int32, device=scores.device)
    cnt = torch.zeros((n1,), dtype=torch.int32, device=scores.device)
    if n1 == 0:
        return out, cnt
    use_min = min_score is not None
    native.check(native.lib().gtsfm_retrieval_pairs(_ptr(scores), n1, n2, _ptr(inv), int(num_select),
                                                    float(min_score) if use_min else 0.0, _flag(use_min), _ptr(out),
                                                    _ptr(cnt), native.stream_handle(stream)),
                 "gtsfm_retrieval_pairs")
    return out, cnt


def netvlad_describe(images: torch.Tensor, weights: torch.Tensor, whiten: bool = True,
                     stream: Optional[torch.cuda.Stream] = None, workspace: Optional[torch.Tensor] = None,
                     keep_vlad: bool = False) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """NetVLAD global descriptors of a batch of same-sized (n, H, W, 3) uint8 RGB images (gtsfm_netvlad_batched).

    weights: the packed fp32 blob (gtsfm_amd.frontend.global_descriptor.netvlad_global_descriptor.pack_netvlad_weights).
    Returns (desc (n, 4096) f32 or None when whiten is False, vlad (n, 32768) f32 or None unless keep_vlad or
    not whiten): the whitened, L2-normalised descriptor and the NetVLADLayer output before whitening."""
    _check(images, "images", _U8, shape=(None, None, None, None))
    assert images.shape[3] == 3, "NetVLAD takes RGB images (netvlad.py:172: image.shape[1] == 3)"
    L = native.lib()
    _check(weights, "weights", _F32, numel=L.gtsfm_netvlad_weights_floats())
    n, H, W = images.shape[0], images.shape[1], images.shape[2]
    dev = images.device
    desc = torch.empty((n, 4096), dtype=torch.float32, device=dev) if whiten else None
    vlad = torch.empty((n, 32768), dtype=torch.float32, device=dev) if (keep_vlad or not whiten) else None
    if n == 0:
        return desc, vlad
    ws = _take_workspace(L.gtsfm_netvlad_workspace_bytes(n, H, W), dev, workspace, stream)
    rc = L.gtsfm_netvlad_batched(_ptr(images), n, H, W, 3, _ptr(weights), _flag(whiten), _ptr(vlad), _ptr(desc),
                                 _ptr(ws), ws.numel(), native.stream_handle(stream))
    native.check(rc, "gtsfm_netvlad_batched")
    return desc, vlad


def viewgraph_cycle_filter(edges: torch.Tensor, R: torch.Tensor, valid: Optional[torch.Tensor], n_img: int,
                           criterion: int, error_threshold_deg: float, stream: Optional[torch.cuda.Stream] = None,
                           workspace: Optional[torch.Tensor] = None, want_total: bool = True,
                           ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """Cycle-consistent rotation filter over a view graph (gtsfm_viewgraph_cycle_filter).

    edges: (E, 2) int32 (i1 < i2 < n_img, each pair once); R: (E, 3, 3) float64 i2Ri1; valid: (E,) uint8 or None.
    Returns (keep (E,) uint8, agg_error_deg (E,) float64, n_triplets (E,) int32, total_triplets (1,) int64 or None),
    all on the device and in input order."""
    _check(edges, "edges", _I32, shape=(None, 2))
    E = edges.shape[0]
    _check(R, "R", _F64, numel=9 * E)
    _check(valid, "valid", _U8, numel=E, optional=True)
    dev = edges.device
    agg = torch.empty(E, dtype=torch.float64, device=dev)
    n_trip = torch.empty(E, dtype=torch.int32, device=dev)
    keep = torch.empty(E, dtype=torch.uint8, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev) if want_total else None
    L = native.lib()
    ws = _take_workspace(L.gtsfm_viewgraph_workspace_bytes(int(n_img), E), dev, workspace, stream, None if E == 0 else
                         f"gtsfm_viewgraph_cycle_filter supports 1..{native.VG_MAX_IMAGES} images, got {n_img}")
    rc = L.gtsfm_viewgraph_cycle_filter(_ptr(edges), _ptr(R), _ptr(valid), int(n_img), E, int(criterion),
                                        float(error_threshold_deg), _ptr(ws), ws.numel(), _ptr(agg), _ptr(n_trip),
                                        _ptr(keep), _ptr(total), native.stream_handle(stream))
    native.check(rc, "gtsfm_viewgraph_cycle_filter")
    return keep, agg, n_trip, total


def tracks_from_matches(pairs: torch.Tensor, offsets: torch.Tensor, v_corr: torch.Tensor, kp_count: torch.Tensor,
                        kmax: int, valid: Optional[torch.Tensor] = None, kp_xy: Optional[torch.Tensor] = None,
                        n_rows: Optional[int] = None, track_cap: Optional[int] = None, meas_cap: Optional[int] = None,
                        stream: Optional[torch.cuda.Stream] = None, workspace: Optional[torch.Tensor] = None,
                        out: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor, Optional[torch.Tensor]]] = None,
                        ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, Optional[torch.Tensor], torch.Tensor]:
    """2D feature tracks of a set of verified correspondences (gtsfm_tracks_from_matches).

    pairs: (P, 2) int32 image indices; offsets: (P + 1,) int32 and v_corr: (rows, 2) int32 holding uint32 keypoint
    indices, the CSR compact_verified returns; kp_count: (n_img,) int32; valid: (P,) uint8 or None; kp_xy:
    (n_img, kmax, 2) float32 or None. n_rows: the rows of v_corr that may be read (default: all of v_corr; the rows in
    use are offsets[P], which stays on the device). track_cap / meas_cap default to min(2 * n_rows, n_img * kmax), which
    always suffices. `out` = (track_offsets, track_img, track_kp, track_uv) reuses the caller's buffers.
    Returns (track_offsets (track_cap + 1,) int32, track_img (meas_cap,) int32, track_kp (meas_cap,) int32, track_uv
    (meas_cap, 2) float32 or None, stats (5,) int64 = n_tracks, n_measurements, n_components, n_erroneous, n_bad_rows),
    all on the device; entries past the counts in stats are not written. Tracks are in canonical order: ascending
    smallest (image, keypoint), measurements ascending inside a track."""
    _check(pairs, "pairs", _I32, shape=(None, 2))
    P = pairs.shape[0]
    _check(offsets, "offsets", _I32, min_numel=P + 1)
    _check(v_corr, "v_corr", _I32, shape=(None, 2))
    _check(kp_count, "kp_count", _I32)
    n_img, kmax = kp_count.numel(), int(kmax)
    _check(valid, "valid", _U8, numel=P, optional=True)
    _check(kp_xy, "kp_xy", _F32, numel=n_img * kmax * 2, optional=True)
    n_rows = v_corr.shape[0] if n_rows is None else int(n_rows)
    assert 0 <= n_rows <= v_corr.shape[0]
    dev = pairs.device
    enough = min(2 * n_rows, n_img * kmax)
    track_cap = enough if track_cap is None else int(track_cap)
    meas_cap = enough if meas_cap is None else int(meas_cap)
    if out is not None:
        t_off, t_img, t_kp, t_uv = out
        assert t_off.numel() >= track_cap + 1 and t_img.numel() >= meas_cap and t_kp.numel() >= meas_cap
        assert t_uv is None or t_uv.numel() >= 2 * meas_cap
    else:
        t_off = torch.empty(track_cap + 1, dtype=torch.int32, device=dev)
        t_img = torch.empty(meas_cap, dtype=torch.int32, device=dev)
        t_kp = torch.empty(meas_cap, dtype=torch.int32, device=dev)
        t_uv = torch.empty((meas_cap, 2), dtype=torch.float32, device=dev) if kp_xy is not None else None
    stats = torch.empty(5, dtype=torch.int64, device=dev)
    L = native.lib()
    ws = _take_workspace(L.gtsfm_tracks_workspace_bytes(n_img, kmax, P, n_rows), dev, workspace, stream,
                         None if P == 0 or n_rows == 0 else
                         f"gtsfm_tracks_from_matches needs 0 < n_img * kmax < 2^31, got {n_img} x {kmax}")
    rc = L.gtsfm_tracks_from_matches(_ptr(pairs), _ptr(offsets), _ptr(v_corr), _ptr(valid), P, n_rows, _ptr(kp_count),
                                     _ptr(kp_xy), n_img, kmax, _ptr(ws), ws.numel(), _ptr(t_off), track_cap,
                                     _ptr(t_img), _ptr(t_kp), _ptr(t_uv), meas_cap, _ptr(stats),
                                     native.stream_handle(stream))
    native.check(rc, "gtsfm_tracks_from_matches")
    return t_off, t_img, t_kp, t_uv, stats


@dataclass(eq=False)
class TriangulationResult:
    """Per-track outputs of triangulate_tracks, all on the device: exit_code (T,) int32, point (T, 3) float64 (NaN
    where the final triangulation did not succeed), avg_err (T,) float64, inlier (n_meas,) uint8, stats (8,) int64 in
    the order of native.TRI_STATS_FIELDS, and, when asked for, n_hyp (T,) int32 and hyp_pair (hyp_cap,) int64."""

    exit_code: torch.Tensor
    point: torch.Tensor
    avg_err: torch.Tensor
    inlier: torch.Tensor
    stats: torch.Tensor
    n_hyp: Optional[torch.Tensor] = None
    hyp_pair: Optional[torch.Tensor] = None


def triangulate_tracks(track_offsets: torch.Tensor, track_img: torch.Tensor, track_uv: torch.Tensor,
                       wRc: torch.Tensor, wtc: torch.Tensor, intrinsics: torch.Tensor,
                       cam_valid: Optional[torch.Tensor], mode: int, reproj_error_threshold: float,
                       min_triangulation_angle: float = 0.0, n_hyp: int = 0, seed: int = 0,
                       n_tracks: Optional[int] = None, n_tracks_dev: Optional[torch.Tensor] = None,
                       track_id: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None,
                       workspace: Optional[torch.Tensor] = None, workspace_bytes: Optional[int] = None,
                       want_hypotheses: bool = False, hyp_cap: Optional[int] = None) -> TriangulationResult:
    """Triangulates every track of a CSR (gtsfm_triangulate_tracks; semantics in include/gtsfm_hip.h).

    track_offsets (>= T + 1,) int32, track_img (n_meas,) int32 and track_uv (n_meas, 2) float32 or float64: the
    arrays tracks_from_matches returns (float32) or a host-built track (float64). n_tracks defaults to
    track_offsets.numel() - 1; n_tracks_dev, an int64 device tensor whose first entry is the track count (the stats of
    tracks_from_matches), makes n_tracks a capacity, so that the chain needs no host synchronisation. wRc (n_img, 3,
    3), wtc (n_img, 3), intrinsics (n_img, 3) float64, cam_valid (n_img,) uint8 or None. mode is a
    native.GTSFM_TRI_* value. workspace_bytes below the query's value forces more chunks (tests)."""
    T, n_meas, uv_is_f64 = _track_csr(track_offsets, track_img, track_uv, n_tracks, n_tracks_dev)
    # unlike global_ba and transavg_measurements, an empty track_offsets is refused unless n_tracks says 0
    assert n_tracks is not None or track_offsets.numel() > 0, "track_offsets is empty"
    n_img = _check_cameras(wRc, wtc, intrinsics, cam_valid)
    _check(track_id, "track_id", _I32, min_numel=T, optional=True)
    if mode == native.GTSFM_TRI_RANSAC_SAMPLE_BIASED_BASELINE:
        raise NotImplementedError("RANSAC_SAMPLE_BIASED_BASELINE (a weighted draw without replacement) is not built")
    n_hyp = min(int(n_hyp), 2 ** 31 - 1)
    dev = track_offsets.device
    exit_code = torch.empty(T, dtype=torch.int32, device=dev)
    point = torch.full((T, 3), float("nan"), dtype=torch.float64, device=dev)
    avg_err = torch.empty(T, dtype=torch.float64, device=dev)
    inlier = torch.zeros(n_meas, dtype=torch.uint8, device=dev)
    stats = torch.empty(8, dtype=torch.int64, device=dev)
    t_n_hyp = hyp_pair = None
    if want_hypotheses:
        t_n_hyp = torch.zeros(T, dtype=torch.int32, device=dev)
        hyp_cap = T * n_hyp if hyp_cap is None else int(hyp_cap)
        hyp_pair = torch.full((max(hyp_cap, 1),), -1, dtype=torch.int64, device=dev)
    L = native.lib()
    need = L.gtsfm_triangulate_workspace_bytes(T, n_meas, n_hyp)
    if workspace_bytes is not None:
        need = int(workspace_bytes)
    ws = _take_workspace(need, dev, workspace, stream)
    rc = L.gtsfm_triangulate_tracks(_ptr(track_offsets), _ptr(track_img), _ptr(track_uv), uv_is_f64, _ptr(track_id), T,
                                    _ptr(n_tracks_dev), n_meas, _ptr(wRc), _ptr(wtc), _ptr(intrinsics),
                                    _ptr(cam_valid), n_img, int(mode), float(reproj_error_threshold),
                                    float(min_triangulation_angle), n_hyp, _u64(seed), _ptr(ws),
                                    need if workspace_bytes is not None else ws.numel(), _ptr(exit_code), _ptr(point),
                                    _ptr(avg_err), _ptr(inlier), _ptr(stats), _ptr(t_n_hyp), _ptr(hyp_pair),
                                    0 if hyp_pair is None else hyp_cap, native.stream_handle(stream))
    native.check(rc, "gtsfm_triangulate_tracks")
    return TriangulationResult(exit_code, point, avg_err, inlier, stats, t_n_hyp, hyp_pair)


@dataclass(eq=False)
class GlobalBaResult:
    """Outputs of global_ba, all on the device: wRc (n_img, 3, 3), wtc (n_img, 3), point (T, 3) float64, track_keep
    (T,) and cam_keep (n_img,) uint8, stats (10,) float64 in the order of native.GBA_STATS_FIELDS."""

    wRc: torch.Tensor
    wtc: torch.Tensor
    point: torch.Tensor
    track_keep: torch.Tensor
    cam_keep: torch.Tensor
    stats: torch.Tensor


def _global_ba_prepare(fn: str, n_stats: int, track_offsets, track_img, track_uv, n_tracks, n_tracks_dev, point,
                       check_cameras, track_valid, meas_valid, stream, workspace):
    """What global_ba and global_ba_calib do before their native call `fn`: the argument checks (check_cameras() checks
    the caller's camera arrays and returns n_img), the outputs they share and the workspace. Returns T, n_meas,
    uv_is_f64, n_img, track_valid as uint8, (wRc_out, wtc_out, point_out, track_keep, cam_keep, stats) and the
    workspace."""
    T, n_meas, uv_is_f64 = _track_csr(track_offsets, track_img, track_uv, n_tracks, n_tracks_dev)
    _check(point, "point", _F64, min_numel=3 * T)
    n_img = check_cameras()
    if track_valid is not None and track_valid.dtype == torch.bool:
        track_valid = track_valid.to(torch.uint8)
    _check(track_valid, "track_valid", _U8, min_numel=T, optional=True)
    _check(meas_valid, "meas_valid", _U8, numel=n_meas, optional=True)
    dev = track_offsets.device
    outs = (torch.empty((n_img, 3, 3), dtype=torch.float64, device=dev),
            torch.empty((n_img, 3), dtype=torch.float64, device=dev),
            torch.empty((T, 3), dtype=torch.float64, device=dev),
            torch.empty(T, dtype=torch.uint8, device=dev),
            torch.empty(n_img, dtype=torch.uint8, device=dev),
            torch.empty(n_stats, dtype=torch.float64, device=dev))
    ws = _take_workspace(getattr(native.lib(), fn + "_workspace_bytes")(T, n_meas, n_img), dev, workspace, stream,
                         None if T == 0 or n_meas == 0 or n_img == 0 else
                         f"{fn}: unsupported shape {T} tracks, {n_meas} measurements, {n_img} images")
    return T, n_meas, uv_is_f64, n_img, track_valid, outs, ws


def global_ba(track_offsets: torch.Tensor, track_img: torch.Tensor, track_uv: torch.Tensor, point: torch.Tensor,
              track_valid: Optional[torch.Tensor], meas_valid: Optional[torch.Tensor], wRc: torch.Tensor,
              wtc: torch.Tensor, intrinsics: torch.Tensor, cam_valid: Optional[torch.Tensor], robust: bool = False,
              measurement_sigma: float = 1.0, cam_pose3_prior_sigma: float = 0.1, max_iterations: int = 0,
              pcg_rel_tol: float = 1e-10, pcg_max_iter: int = 2000, reproj_error_thresh: float = float("inf"),
              n_tracks: Optional[int] = None, n_tracks_dev: Optional[torch.Tensor] = None,
              stream: Optional[torch.cuda.Stream] = None, workspace: Optional[torch.Tensor] = None,
              workspace_bytes: Optional[int] = None) -> GlobalBaResult:
    """Bundle-adjusts every camera and landmark of a track CSR (gtsfm_global_ba; semantics in include/gtsfm_hip.h).

    track_offsets / track_img / track_uv as for triangulate_tracks, point (T, 3) float64 its landmarks, track_valid
    (T,) uint8 or bool or None, meas_valid (n_meas,) uint8 or None (the triangulation's inlier bytes). The call runs
    its LM / PCG control flow on the host and synchronises the stream; only those control scalars reach the host.
    workspace_bytes below the query's value is passed as is (tests of the capacity error)."""
    T, n_meas, uv_is_f64, n_img, track_valid, outs, ws = _global_ba_prepare(
        "gtsfm_global_ba", 10, track_offsets, track_img, track_uv, n_tracks, n_tracks_dev, point,
        lambda: _check_cameras(wRc, wtc, intrinsics, cam_valid), track_valid, meas_valid, stream, workspace)
    rc = native.lib().gtsfm_global_ba(
        _ptr(track_offsets), _ptr(track_img), _ptr(track_uv), uv_is_f64, T, _ptr(n_tracks_dev), n_meas, _ptr(point),
        _ptr(track_valid), _ptr(meas_valid), _ptr(wRc), _ptr(wtc), _ptr(intrinsics), _ptr(cam_valid), n_img,
        _flag(robust), float(measurement_sigma), float(cam_pose3_prior_sigma), int(max_iterations),
        float(pcg_rel_tol), int(pcg_max_iter), float(reproj_error_thresh), _ptr(ws),
        ws.numel() if workspace_bytes is None else int(workspace_bytes), *map(_ptr, outs),
        native.stream_handle(stream))
    native.check(rc, "gtsfm_global_ba")
    return GlobalBaResult(*outs)


@dataclass(eq=False)
class GlobalBaCalibResult(GlobalBaResult):
    """Outputs of global_ba_calib: GlobalBaResult's, with stats (12,) in the order of native.GBA_CALIB_STATS_FIELDS, plus
    calib (n_img, 5) float64 = (f, k1, k2, u0, v0), refined for the modelled cameras."""

    calib: torch.Tensor


def global_ba_calib(track_offsets: torch.Tensor, track_img: torch.Tensor, track_uv: torch.Tensor,
                    point: torch.Tensor, track_valid: Optional[torch.Tensor], meas_valid: Optional[torch.Tensor],
                    wRc: torch.Tensor, wtc: torch.Tensor, calib: torch.Tensor, cam_valid: Optional[torch.Tensor],
                    robust: bool = False, measurement_sigma: float = 1.0, cam_pose3_prior_sigma: float = 0.1,
                    shared_calib: bool = False, calibration_prior_sigma: float = 1e-5, max_iterations: int = 0,
                    pcg_rel_tol: float = 1e-10, pcg_max_iter: int = 2000, reproj_error_thresh: float = float("inf"),
                    n_tracks: Optional[int] = None, n_tracks_dev: Optional[torch.Tensor] = None,
                    stream: Optional[torch.cuda.Stream] = None, workspace: Optional[torch.Tensor] = None,
                    workspace_bytes: Optional[int] = None) -> GlobalBaCalibResult:
    """global_ba with the Cal3Bundler calibration (f, k1, k2) refined, one variable per modelled camera or, with
    shared_calib, one for all (gtsfm_global_ba_calib; semantics in include/gtsfm_hip.h).

    The arguments are global_ba's, with calib (n_img, 5) float64 = (f, k1, k2, u0, v0) in place of intrinsics, and the
    prior sigma of the calibration variables. Like global_ba the call synchronises the stream."""
    def check_cameras() -> int:
        n_img = calib.numel() // 5
        _check(wRc, "wRc", _F64, numel=9 * n_img)
        _check(wtc, "wtc", _F64, numel=3 * n_img)
        _check(calib, "calib", _F64, numel=5 * n_img)
        _check(cam_valid, "cam_valid", _U8, numel=n_img, optional=True)
        return n_img

    T, n_meas, uv_is_f64, n_img, track_valid, outs, ws = _global_ba_prepare(
        "gtsfm_global_ba_calib", 12, track_offsets, track_img, track_uv, n_tracks, n_tracks_dev, point,
        check_cameras, track_valid, meas_valid, stream, workspace)
    wRc_out, wtc_out, point_out, track_keep, cam_keep, stats = outs
    calib_out = torch.empty((n_img, 5), dtype=torch.float64, device=track_offsets.device)
    rc = native.lib().gtsfm_global_ba_calib(
        _ptr(track_offsets), _ptr(track_img), _ptr(track_uv), uv_is_f64, T, _ptr(n_tracks_dev), n_meas, _ptr(point),
        _ptr(track_valid), _ptr(meas_valid), _ptr(wRc), _ptr(wtc), _ptr(calib), _ptr(cam_valid), n_img,
        _flag(robust), float(measurement_sigma), float(cam_pose3_prior_sigma), _flag(shared_calib),
        float(calibration_prior_sigma), int(max_iterations), float(pcg_rel_tol), int(pcg_max_iter),
        float(reproj_error_thresh), _ptr(ws), ws.numel() if workspace_bytes is None else int(workspace_bytes),
        _ptr(wRc_out), _ptr(wtc_out), _ptr(calib_out), _ptr(point_out), _ptr(track_keep), _ptr(cam_keep),
        _ptr(stats), native.stream_handle(stream))
    native.check(rc, "gtsfm_global_ba_calib")
    return GlobalBaCalibResult(*outs, calib_out)


@dataclass(eq=False)
class BaInputResult:
    """Outputs of assemble_ba_input, all on the device: cam_keep (n_img,) and track_keep (T,) uint8, track_len (T,)
    int32, stats (6,) int64 in the order of native.BA_INPUT_STATS_FIELDS."""

    cam_keep: torch.Tensor
    track_keep: torch.Tensor
    track_len: torch.Tensor
    stats: torch.Tensor


def assemble_ba_input(track_offsets: torch.Tensor, track_img: torch.Tensor, track_valid: Optional[torch.Tensor],
                      meas_inlier: Optional[torch.Tensor], cam_valid: Optional[torch.Tensor], n_img: int,
                      extra_edges: Optional[torch.Tensor] = None, n_tracks: Optional[int] = None,
                      n_tracks_dev: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None,
                      workspace: Optional[torch.Tensor] = None,
                      workspace_bytes: Optional[int] = None) -> BaInputResult:
    """The cameras and tracks that go into bundle adjustment: the largest connected component of cameras joined by
    the accepted tracks, and the tracks wholly inside it (gtsfm_assemble_ba_input; semantics in include/gtsfm_hip.h).

    track_offsets (>= T + 1,) and track_img (n_meas,) int32 as for triangulate_tracks; track_valid (T,) uint8 or bool
    or None, meas_inlier (n_meas,) uint8 or None (the triangulation's inlier bytes), cam_valid (n_img,) uint8 or None,
    extra_edges (n_extra, 2) int32 or None. Nothing is copied to the host or synchronised. workspace_bytes below the
    query's value is passed as is (tests of the capacity error)."""
    _check(n_tracks_dev, "n_tracks_dev", _I64, min_numel=1, optional=True)
    _check(track_offsets, "track_offsets", _I32)
    _check(track_img, "track_img", _I32)
    n_meas = track_img.numel()
    T = max(track_offsets.numel() - 1, 0) if n_tracks is None else int(n_tracks)
    assert 0 <= T <= max(track_offsets.numel() - 1, 0), f"n_tracks {T} for {track_offsets.numel()} track_offsets"
    n_img = int(n_img)
    if track_valid is not None and track_valid.dtype == torch.bool:
        track_valid = track_valid.to(torch.uint8)
    _check(track_valid, "track_valid", _U8, min_numel=T, optional=True)
    _check(meas_inlier, "meas_inlier", _U8, numel=n_meas, optional=True)
    _check(cam_valid, "cam_valid", _U8, numel=n_img, optional=True)
    _check(extra_edges, "extra_edges", _I32, shape=(None, 2), optional=True)
    n_extra = 0 if extra_edges is None else extra_edges.shape[0]
    dev = track_offsets.device
    cam_keep = torch.empty(n_img, dtype=torch.uint8, device=dev)
    track_keep = torch.empty(T, dtype=torch.uint8, device=dev)
    track_len = torch.empty(T, dtype=torch.int32, device=dev)
    stats = torch.empty(6, dtype=torch.int64, device=dev)
    L = native.lib()
    ws = _take_workspace(L.gtsfm_assemble_ba_input_workspace_bytes(T, n_img), dev, workspace, stream,
                         None if T == 0 or n_img == 0 else
                         f"gtsfm_assemble_ba_input: unsupported shape {T} tracks, {n_img} images")
    rc = L.gtsfm_assemble_ba_input(_ptr(track_offsets), _ptr(track_img), T, _ptr(n_tracks_dev), n_meas,
                                   _ptr(track_valid), _ptr(meas_inlier), _ptr(cam_valid), n_img,
                                   _ptr(extra_edges) if n_extra else None, n_extra, _ptr(ws),
                                   ws.numel() if workspace_bytes is None else int(workspace_bytes), _ptr(cam_keep),
                                   _ptr(track_keep), _ptr(track_len), _ptr(stats), native.stream_handle(stream))
    native.check(rc, "gtsfm_assemble_ba_input")
    return BaInputResult(cam_keep, track_keep, track_len, stats)


@dataclass(eq=False)
class TransAvgMeasurements:
    """Outputs of transavg_measurements, all on the device: key (n_edges + n_meas, 2) int32, dir (.., 3) float64, valid
    (..,) uint8, selected (n_tracks,) int32, cam_valid (n_img,) uint8, counts (4,) int64 = valid camera edges, track
    slots in use, selected tracks, track measurements in a camera without rotation."""

    key: torch.Tensor
    dir: torch.Tensor
    valid: torch.Tensor
    selected: torch.Tensor
    cam_valid: torch.Tensor
    counts: torch.Tensor
    n_edges: int


def transavg_measurements(edges: torch.Tensor, i2Ui1: torch.Tensor, edge_valid: Optional[torch.Tensor],
                          wRi: torch.Tensor, rot_valid: Optional[torch.Tensor],
                          track_offsets: Optional[torch.Tensor] = None, track_img: Optional[torch.Tensor] = None,
                          track_uv: Optional[torch.Tensor] = None, intrinsics: Optional[torch.Tensor] = None,
                          measurements_per_camera: int = 12, n_tracks: Optional[int] = None,
                          n_tracks_dev: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None,
                          workspace: Optional[torch.Tensor] = None) -> TransAvgMeasurements:
    """World-frame direction measurements and track selection of 1DSfM (gtsfm_transavg_measurements; semantics in
    include/gtsfm_hip.h). edges (E, 2) int32 = (i1, i2), i2Ui1 (E, 3) float64, wRi (n_img, 3, 3) float64, the valid
    masks uint8 or None; the track CSR as tracks_from_matches returns it (or None: camera edges only)."""
    _check(edges, "edges", _I32, shape=(None, 2))
    E = edges.shape[0]
    n_img = wRi.numel() // 9
    assert E > 0 and n_img > 0, f"{E} edges, {n_img} images"
    _check(i2Ui1, "i2Ui1", _F64, numel=3 * E)
    _check(wRi, "wRi", _F64, numel=9 * n_img)
    _check(edge_valid, "edge_valid", _U8, numel=E, optional=True)
    _check(rot_valid, "rot_valid", _U8, numel=n_img, optional=True)
    dev = edges.device
    T, n_meas, uv_is_f64 = _track_csr(track_offsets, track_img, track_uv, n_tracks, n_tracks_dev)
    if track_offsets is not None:
        _check(intrinsics, "intrinsics", _F64, numel=3 * n_img)
    key = torch.empty((E + n_meas, 2), dtype=torch.int32, device=dev)
    dirs = torch.empty((E + n_meas, 3), dtype=torch.float64, device=dev)
    valid = torch.empty(E + n_meas, dtype=torch.uint8, device=dev)
    selected = torch.empty(max(T, 1), dtype=torch.int32, device=dev)
    cam_valid = torch.empty(n_img, dtype=torch.uint8, device=dev)
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    L = native.lib()
    ws = _take_workspace(L.gtsfm_transavg_measurements_workspace_bytes(E, T, n_meas, n_img), dev, workspace, stream,
                         f"gtsfm_transavg_measurements: unsupported shape {E} edges, {T} tracks, {n_img} images")
    rc = L.gtsfm_transavg_measurements(_ptr(edges), _ptr(i2Ui1), _ptr(edge_valid), E, _ptr(wRi), _ptr(rot_valid), n_img,
                                       _ptr(track_offsets), _ptr(track_img), _ptr(track_uv), uv_is_f64, T,
                                       _ptr(n_tracks_dev), n_meas, _ptr(intrinsics), int(measurements_per_camera),
                                       _ptr(ws), ws.numel(), _ptr(key), _ptr(dirs), _ptr(valid), _ptr(selected),
                                       _ptr(cam_valid), _ptr(counts), native.stream_handle(stream))
    native.check(rc, "gtsfm_transavg_measurements")
    return TransAvgMeasurements(key, dirs, valid, selected[:T], cam_valid, counts, E)


def transavg_mfas(key: torch.Tensor, dirs: torch.Tensor, valid: Optional[torch.Tensor], n_nodes: int,
                  proj: torch.Tensor, threshold: float = 0.125, want_violated: bool = False,
                  stream: Optional[torch.cuda.Stream] = None, workspace: Optional[torch.Tensor] = None,
                  ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """MFAS outlier weights over every projection direction in one launch (gtsfm_transavg_mfas). key (n, 2) int32,
    dirs (n, 3) float64, valid (n,) uint8 or None, proj (n_dir, 3) float64. Returns (outlier_sum (n,) float64, inlier
    (n,) uint8, violated (n_dir, ceil(n / 32)) int32 holding the uint32 bit words, or None)."""
    _check(key, "key", _I32, shape=(None, 2))
    n = key.shape[0]
    _check(dirs, "dirs", _F64, numel=3 * n)
    _check(proj, "proj", _F64, shape=(None, None))
    n_dir = proj.shape[0]
    _check(valid, "valid", _U8, numel=n, optional=True)
    if n_nodes > native.TA_MFAS_MAX_NODES:
        raise native.NativeError(f"gtsfm_transavg_mfas holds its node state in LDS: {n_nodes} nodes exceed "
                                 f"{native.TA_MFAS_MAX_NODES}")
    dev = key.device
    osum = torch.empty(n, dtype=torch.float64, device=dev)
    inlier = torch.empty(n, dtype=torch.uint8, device=dev)
    viol = torch.empty((n_dir, (n + 31) // 32), dtype=torch.int32, device=dev) if want_violated else None
    L = native.lib()
    ws = _take_workspace(L.gtsfm_transavg_mfas_workspace_bytes(n, int(n_nodes), n_dir), dev, workspace, stream,
                         f"gtsfm_transavg_mfas: unsupported shape {n} measurements, {n_nodes} nodes, {n_dir} "
                         "directions")
    rc = L.gtsfm_transavg_mfas(_ptr(key), _ptr(dirs), _ptr(valid), n, int(n_nodes), _ptr(proj), n_dir, float(threshold),
                               _ptr(ws), ws.numel(), _ptr(osum), _ptr(inlier), _ptr(viol), native.stream_handle(stream))
    native.check(rc, "gtsfm_transavg_mfas")
    return osum, inlier, viol


@dataclass(eq=False)
class TransAvgResult:
    """Outputs of transavg_recover, all on the device: wti (n_img, 3) float64, wti_valid (n_img,) uint8, landmark
    (n_landmarks, 3), landmark_valid, stats (10,) float64 in the order of native.TA_STATS_FIELDS."""

    wti: torch.Tensor
    wti_valid: torch.Tensor
    landmark: torch.Tensor
    landmark_valid: torch.Tensor
    stats: torch.Tensor


def transavg_recover(key: torch.Tensor, dirs: torch.Tensor, inlier: torch.Tensor, n_img: int, n_landmarks: int,
                     rot_valid: Optional[torch.Tensor] = None, robust: bool = True, scale: float = 1.0, seed: int = 0,
                     max_iterations: int = 0, pcg_rel_tol: float = 1e-10, pcg_max_iter: int = 2000,
                     stream: Optional[torch.cuda.Stream] = None, workspace: Optional[torch.Tensor] = None,
                     ) -> TransAvgResult:
    """Camera and landmark positions from the inlier direction measurements (gtsfm_transavg_recover). Runs its LM / PCG
    control flow on the host and synchronises the stream."""
    _check(key, "key", _I32, shape=(None, 2))
    n = key.shape[0]
    _check(dirs, "dirs", _F64, numel=3 * n)
    _check(inlier, "inlier", _U8, numel=n)
    _check(rot_valid, "rot_valid", _U8, numel=n_img, optional=True)
    dev = key.device
    wti = torch.empty((n_img, 3), dtype=torch.float64, device=dev)
    wti_valid = torch.empty(n_img, dtype=torch.uint8, device=dev)
    land = torch.empty((n_landmarks, 3), dtype=torch.float64, device=dev)
    land_valid = torch.empty(n_landmarks, dtype=torch.uint8, device=dev)
    stats = torch.empty(10, dtype=torch.float64, device=dev)
    L = native.lib()
    ws = _take_workspace(L.gtsfm_transavg_recover_workspace_bytes(n, int(n_img), int(n_landmarks)), dev, workspace,
                         stream, f"gtsfm_transavg_recover: unsupported shape {n} measurements, {n_img} images, "
                         f"{n_landmarks} landmarks")
    rc = L.gtsfm_transavg_recover(_ptr(key), _ptr(dirs), _ptr(inlier), n, int(n_img), int(n_landmarks), _ptr(rot_valid),
                                  _flag(robust), float(scale), _u64(seed), int(max_iterations),
                                  float(pcg_rel_tol), int(pcg_max_iter), _ptr(ws), ws.numel(), _ptr(wti),
                                  _ptr(wti_valid), _ptr(land) if n_landmarks else None,
                                  _ptr(land_valid) if n_landmarks else None, _ptr(stats), native.stream_handle(stream))
    native.check(rc, "gtsfm_transavg_recover")
    return TransAvgResult(wti, wti_valid, land, land_valid, stats)


@dataclass(eq=False)
class RotAvgResult:
    """Outputs of rotavg_shonan, all on the device: wRi (n_img, 3, 3) float64 (zero where invalid), rot_valid (n_img,)
    uint8, stats (12,) float64 in the order of native.RA_STATS_FIELDS."""

    wRi: torch.Tensor
    rot_valid: torch.Tensor
    stats: torch.Tensor


def rotavg_shonan(edges: torch.Tensor, aRb: torch.Tensor, kappa: Optional[torch.Tensor], edge_valid: Optional[torch.Tensor],
                  n_img: int, wRi_init: Optional[torch.Tensor] = None, seed: int = 0, p_min: int = 5, p_max: int = 30,
                  optimality_threshold: float = -1e-4, grad_rel_tol: float = 1e-10, max_iterations: int = 100,
                  pcg_rel_tol: float = 1e-2, pcg_max_iter: int = 200, eig_tol: float = 1e-8, eig_max_steps: int = 4000,
                  stream: Optional[torch.cuda.Stream] = None, workspace: Optional[torch.Tensor] = None,
                  ) -> RotAvgResult:
    """Global rotations from relative ones by Shonan averaging with an optimality certificate (gtsfm_rotavg_shonan).
    edges (E, 2) int32 = (a, b) with aRb (E, 3, 3) float64 asking wRa aRb = wRb; kappa (E,) float64 or None (= 1).
    Runs its LM / PCG / Lanczos control flow on the host and synchronises the stream."""
    _check(edges, "edges", _I32, shape=(None, 2))
    n = edges.shape[0]
    _check(aRb, "aRb", _F64, numel=9 * n)
    _check(kappa, "kappa", _F64, numel=n, optional=True)
    _check(edge_valid, "edge_valid", _U8, numel=n, optional=True)
    _check(wRi_init, "wRi_init", _F64, numel=9 * n_img, optional=True)
    dev = edges.device
    wRi = torch.empty((n_img, 3, 3), dtype=torch.float64, device=dev)
    rot_valid = torch.empty(n_img, dtype=torch.uint8, device=dev)
    stats = torch.empty(12, dtype=torch.float64, device=dev)
    L = native.lib()
    ws = _take_workspace(L.gtsfm_rotavg_workspace_bytes(n, int(n_img), int(p_max)), dev, workspace, stream,
                         f"gtsfm_rotavg_shonan: unsupported shape {n} edges, {n_img} images, p_max {p_max}")
    rc = L.gtsfm_rotavg_shonan(_ptr(edges), _ptr(aRb), _ptr(kappa), _ptr(edge_valid), n, int(n_img), _ptr(wRi_init),
                               _u64(seed), int(p_min), int(p_max), float(optimality_threshold),
                               float(grad_rel_tol), int(max_iterations), float(pcg_rel_tol), int(pcg_max_iter),
                               float(eig_tol), int(eig_max_steps), _ptr(ws), ws.numel(), _ptr(wRi), _ptr(rot_valid),
                               _ptr(stats), native.stream_handle(stream))
    native.check(rc, "gtsfm_rotavg_shonan")
    return RotAvgResult(wRi, rot_valid, stats)


@dataclass(eq=False)
class MvsViewsResult:
    """Outputs of mvs_select_views, all on the device and sized by n_img (the caller slices by stats[0] = n_valid):
    img_to_pm and pm_to_img (n_img,) int32, scores (n_img, n_img) int64 in units of 2^-40, src_views (n_img,
    max_num_views - 1) int32, depth_range (n_img, 2) float64, stats (4,) int64 in the order of
    native.MVS_VIEWS_STATS_FIELDS."""

    img_to_pm: torch.Tensor
    pm_to_img: torch.Tensor
    scores: torch.Tensor
    src_views: torch.Tensor
    depth_range: torch.Tensor
    stats: torch.Tensor


def mvs_select_views(track_offsets: torch.Tensor, track_img: torch.Tensor, point: torch.Tensor,
                     track_keep: Optional[torch.Tensor], meas_inlier: Optional[torch.Tensor], wRc: torch.Tensor,
                     wtc: torch.Tensor, cam_keep: Optional[torch.Tensor], max_num_views: int = 5,
                     n_tracks: Optional[int] = None, stream: Optional[torch.cuda.Stream] = None,
                     workspace: Optional[torch.Tensor] = None,
                     workspace_bytes: Optional[int] = None) -> MvsViewsResult:
    """Source views and depth ranges of every valid camera from the tracks (gtsfm_mvs_select_views; semantics in
    include/gtsfm_hip.h). Nothing is copied to the host or synchronised. workspace_bytes below the query's value is
    passed as is (tests of the capacity error)."""
    _check(track_offsets, "track_offsets", _I32)
    _check(track_img, "track_img", _I32)
    n_meas = track_img.numel()
    T = max(track_offsets.numel() - 1, 0) if n_tracks is None else int(n_tracks)
    assert 0 <= T <= max(track_offsets.numel() - 1, 0), f"n_tracks {T} for {track_offsets.numel()} track_offsets"
    n_img = wtc.numel() // 3
    _check(wRc, "wRc", _F64, numel=9 * n_img)
    _check(wtc, "wtc", _F64, numel=3 * n_img)
    _check(point, "point", _F64, min_numel=3 * T)
    if track_keep is not None and track_keep.dtype == torch.bool:
        track_keep = track_keep.to(torch.uint8)
    _check(track_keep, "track_keep", _U8, min_numel=T, optional=True)
    _check(meas_inlier, "meas_inlier", _U8, numel=n_meas, optional=True)
    _check(cam_keep, "cam_keep", _U8, numel=n_img, optional=True)
    S = int(max_num_views) - 1
    dev = wtc.device
    r = MvsViewsResult(torch.empty(n_img, dtype=_I32, device=dev), torch.empty(n_img, dtype=_I32, device=dev),
                       torch.empty((n_img, n_img), dtype=_I64, device=dev),
                       torch.empty((n_img, max(S, 0)), dtype=_I32, device=dev),
                       torch.empty((n_img, 2), dtype=_F64, device=dev), torch.empty(4, dtype=_I64, device=dev))
    L = native.lib()
    ws = _take_workspace(L.gtsfm_mvs_select_views_workspace_bytes(T, n_meas, n_img), dev, workspace, stream,
                         None if T == 0 or n_meas == 0 or n_img == 0 else
                         f"gtsfm_mvs_select_views: unsupported shape {T} tracks, {n_meas} measurements, {n_img} images")
    rc = L.gtsfm_mvs_select_views(_ptr(track_offsets), _ptr(track_img), T, n_meas, _ptr(point), _ptr(track_keep),
                                  _ptr(meas_inlier), _ptr(wRc), _ptr(wtc), _ptr(cam_keep), n_img, int(max_num_views),
                                  _ptr(ws), ws.numel() if workspace_bytes is None else int(workspace_bytes),
                                  _ptr(r.img_to_pm), _ptr(r.pm_to_img), _ptr(r.scores),
                                  _ptr(r.src_views) if S > 0 else None, _ptr(r.depth_range), _ptr(r.stats),
                                  native.stream_handle(stream))
    native.check(rc, "gtsfm_mvs_select_views")
    return r


@dataclass(eq=False)
class MvsFusedResult:
    """Outputs of mvs_fuse_depth, all on the device: fused (n, H, W) float32, mask (n, H, W) uint8 (bit 0 geometric,
    bit 1 confidence, bit 2 joint), counts (n, 4) int64 in the order of native.MVS_FUSE_COUNT_FIELDS, err (n, 3)
    float64 = (sum, min, max) of the counted reprojection errors."""

    fused: torch.Tensor
    mask: torch.Tensor
    counts: torch.Tensor
    err: torch.Tensor


def mvs_fuse_depth(depth: torch.Tensor, confidence: torch.Tensor, wRc: torch.Tensor, wtc: torch.Tensor,
                   intrinsics: torch.Tensor, src_views: torch.Tensor, pixel_thresh: float = 1.0,
                   depth_thresh: float = 0.01, min_confidence: float = 0.8, min_consistent_views: int = 1,
                   stream: Optional[torch.cuda.Stream] = None, workspace: Optional[torch.Tensor] = None,
                   workspace_bytes: Optional[int] = None) -> MvsFusedResult:
    """Geometric-consistency filter and fusion of the depth maps of all views (gtsfm_mvs_fuse_depth). depth and
    confidence (n, H, W) float32, cameras per view, src_views (n, S) int32. Nothing is copied to the host or
    synchronised."""
    _check(depth, "depth", _F32, shape=(None, None, None))
    n, H, W = depth.shape
    _check(confidence, "confidence", _F32, shape=(n, H, W))
    assert _check_cameras(wRc, wtc, intrinsics, None) == n, f"{intrinsics.numel() // 3} cameras for {n} views"
    _check(src_views, "src_views", _I32, shape=(n, None))
    S = src_views.shape[1]
    dev = depth.device
    r = MvsFusedResult(torch.empty((n, H, W), dtype=_F32, device=dev), torch.empty((n, H, W), dtype=_U8, device=dev),
                       torch.empty((n, 4), dtype=_I64, device=dev), torch.empty((n, 3), dtype=_F64, device=dev))
    L = native.lib()
    ws = _take_workspace(L.gtsfm_mvs_fuse_depth_workspace_bytes(n, H, W), dev, workspace, stream,
                         None if n == 0 or H == 0 or W == 0 else
                         f"gtsfm_mvs_fuse_depth: unsupported shape {n} views of {H} x {W}")
    rc = L.gtsfm_mvs_fuse_depth(_ptr(depth), _ptr(confidence), n, H, W, _ptr(wRc), _ptr(wtc), _ptr(intrinsics),
                                _ptr(src_views) if S else None, S, float(pixel_thresh), float(depth_thresh),
                                float(min_confidence), int(min_consistent_views), _ptr(ws),
                                ws.numel() if workspace_bytes is None else int(workspace_bytes), _ptr(r.fused),
                                _ptr(r.mask), _ptr(r.counts), _ptr(r.err), native.stream_handle(stream))
    native.check(rc, "gtsfm_mvs_fuse_depth")
    return r


def mvs_gather_points(fused: torch.Tensor, mask: torch.Tensor, wRc: torch.Tensor, wtc: torch.Tensor,
                      intrinsics: torch.Tensor, images: torch.Tensor, view_image: Optional[torch.Tensor],
                      capacity: int, stream: Optional[torch.cuda.Stream] = None,
                      workspace: Optional[torch.Tensor] = None, workspace_bytes: Optional[int] = None,
                      ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The coloured points of the joint pixels in canonical order (gtsfm_mvs_gather_points): views ascending, then
    row-major. images (n_images, h, w, 3) uint8 with h >= H and w >= W, view_image (n,) int32 or None. Returns points
    (capacity, 3) float64, colors (capacity, 3) uint8 and view_offset (n + 1,) int64; capacity is the caller's, read
    from mvs_fuse_depth's counts. Nothing is copied to the host or synchronised."""
    _check(fused, "fused", _F32, shape=(None, None, None))
    n, H, W = fused.shape
    _check(mask, "mask", _U8, shape=(n, H, W))
    assert _check_cameras(wRc, wtc, intrinsics, None) == n, f"{intrinsics.numel() // 3} cameras for {n} views"
    _check(images, "images", _U8, shape=(None, None, None, 3))
    _check(view_image, "view_image", _I32, numel=n, optional=True)
    capacity = int(capacity)
    dev = fused.device
    points = torch.empty((max(capacity, 0), 3), dtype=_F64, device=dev)
    colors = torch.empty((max(capacity, 0), 3), dtype=_U8, device=dev)
    view_offset = torch.empty(n + 1, dtype=_I64, device=dev)
    L = native.lib()
    ws = _take_workspace(L.gtsfm_mvs_gather_points_workspace_bytes(n, H, W), dev, workspace, stream,
                         None if n == 0 or H == 0 or W == 0 else
                         f"gtsfm_mvs_gather_points: unsupported shape {n} views of {H} x {W}")
    rc = L.gtsfm_mvs_gather_points(_ptr(fused), _ptr(mask), n, H, W, _ptr(wRc), _ptr(wtc), _ptr(intrinsics),
                                   _ptr(images), _ptr(view_image), images.shape[0], images.shape[1], images.shape[2],
                                   capacity, _ptr(ws), ws.numel() if workspace_bytes is None else int(workspace_bytes),
                                   _ptr(points) if capacity > 0 else None, _ptr(colors) if capacity > 0 else None,
                                   _ptr(view_offset), native.stream_handle(stream))
    native.check(rc, "gtsfm_mvs_gather_points")
    return points, colors, view_offset


def mvs_voxel_stats(points: torch.Tensor, stream: Optional[torch.cuda.Stream] = None,
                    workspace: Optional[torch.Tensor] = None, workspace_bytes: Optional[int] = None) -> torch.Tensor:
    """(18,) float64 on the device: mean, scatter / (N - 1), min and max bound of points (N, 3) float64
    (gtsfm_mvs_voxel_stats)."""
    _check(points, "points", _F64, shape=(None, 3))
    n = points.shape[0]
    stats = torch.empty(18, dtype=_F64, device=points.device)
    L = native.lib()
    ws = _take_workspace(L.gtsfm_mvs_voxel_stats_workspace_bytes(n), points.device, workspace, stream)
    rc = L.gtsfm_mvs_voxel_stats(_ptr(points), n, _ptr(ws), ws.numel() if workspace_bytes is None else
                                 int(workspace_bytes), _ptr(stats), native.stream_handle(stream))
    native.check(rc, "gtsfm_mvs_voxel_stats")
    return stats


@dataclass(eq=False)
class MvsVoxelResult:
    """Outputs of mvs_voxel_downsample, all on the device with N rows of which the first n_voxels[0] are used: points
    (N, 3) float64, colors (N, 3) uint8, keys (N,) int64 ascending, count (N,) int32, n_voxels (1,) int64."""

    points: torch.Tensor
    colors: torch.Tensor
    keys: torch.Tensor
    count: torch.Tensor
    n_voxels: torch.Tensor


def mvs_voxel_downsample(points: torch.Tensor, colors: torch.Tensor, stats: torch.Tensor, voxel_size: float,
                         stream: Optional[torch.cuda.Stream] = None, workspace: Optional[torch.Tensor] = None,
                         workspace_bytes: Optional[int] = None) -> MvsVoxelResult:
    """One point per occupied voxel, in ascending key order: gtsfm_mvs_voxel_keys, a stable torch.sort of the keys
    (plumbing) and gtsfm_mvs_voxel_downsample's segmented mean. stats is mvs_voxel_stats' result (its min bound is the
    grid's origin); voxel_size > 0. Nothing is copied to the host or synchronised."""
    _check(points, "points", _F64, shape=(None, 3))
    n = points.shape[0]
    _check(colors, "colors", _U8, shape=(n, 3))
    _check(stats, "stats", _F64, numel=18)
    dev = points.device
    L = native.lib()
    keys = torch.empty(n, dtype=_I64, device=dev)
    native.check(L.gtsfm_mvs_voxel_keys(_ptr(points), n, _ptr(stats), float(voxel_size), _ptr(keys),
                                        native.stream_handle(stream)), "gtsfm_mvs_voxel_keys")
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        sorted_keys, perm = torch.sort(keys, stable=True)  # on the stream of the two calls around it
    r = MvsVoxelResult(torch.empty((n, 3), dtype=_F64, device=dev), torch.empty((n, 3), dtype=_U8, device=dev),
                       torch.empty(n, dtype=_I64, device=dev), torch.empty(n, dtype=_I32, device=dev),
                       torch.empty(1, dtype=_I64, device=dev))
    ws = _take_workspace(L.gtsfm_mvs_voxel_downsample_workspace_bytes(n), dev, workspace, stream)
    rc = L.gtsfm_mvs_voxel_downsample(_ptr(points), _ptr(colors), _ptr(sorted_keys), _ptr(perm), n, _ptr(ws),
                                      ws.numel() if workspace_bytes is None else int(workspace_bytes), _ptr(r.points),
                                      _ptr(r.colors), _ptr(r.keys), _ptr(r.count), _ptr(r.n_voxels),
                                      native.stream_handle(stream))
    native.check(rc, "gtsfm_mvs_voxel_downsample")
    return r


@dataclass(eq=False)
class PatchmatchNetResult:
    """Outputs of patchmatchnet_depth, all on the device: depth and confidence (n, H, W) float32; with debug=True also
    features = the channels-last maps of every view ((n, H/8, W/8, 64), (n, H/4, W/4, 32), (n, H/2, W/2, 16)) and
    iter_depths = the depth after each of the five patchmatch iterations (two (n, H/8, W/8), two (n, H/4, W/4), one
    (n, H/2, W/2)), else None."""

    depth: torch.Tensor
    confidence: torch.Tensor
    features: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None
    iter_depths: Optional[Tuple[torch.Tensor, ...]] = None


def patchmatchnet_depth(images: torch.Tensor, wRc: torch.Tensor, wtc: torch.Tensor, intrinsics: torch.Tensor,
                        src_views: torch.Tensor, depth_range: torch.Tensor, weights: torch.Tensor,
                        init_uniform: torch.Tensor, debug: bool = False,
                        config: Optional[native.PatchmatchNetConfig] = None,
                        stream: Optional[torch.cuda.Stream] = None, workspace: Optional[torch.Tensor] = None
                        ) -> PatchmatchNetResult:
    """PatchmatchNet depth and confidence of every view of a batch (gtsfm_patchmatchnet_batched): images (n, H, W, 3)
    uint8 with H and W multiples of 8, cameras per view, src_views (n, S) int32 rows of the same batch, depth_range
    (n, 2) float64, weights the packed blob (gtsfm_amd.densify.patchmatchnet.pack_patchmatchnet_weights), init_uniform
    (n, 48, H/8, W/8) float32 in [0, 1). Nothing is copied to the host or synchronised."""
    _check(images, "images", _U8, shape=(None, None, None, 3))
    n, H, W = images.shape[:3]
    assert _check_cameras(wRc, wtc, intrinsics, None) == n, f"{intrinsics.numel() // 3} cameras for {n} views"
    _check(src_views, "src_views", _I32, shape=(n, None))
    S = src_views.shape[1]
    _check(depth_range, "depth_range", _F64, shape=(n, 2))
    L = native.lib()
    _check(weights, "weights", _F32, numel=L.gtsfm_patchmatchnet_weights_floats())
    _check(init_uniform, "init_uniform", _F32, shape=(n, native.PATCHMATCHNET_INIT_BINS, H // 8, W // 8))
    dev = images.device
    r = PatchmatchNetResult(torch.empty((n, H, W), dtype=_F32, device=dev),
                            torch.empty((n, H, W), dtype=_F32, device=dev))
    feat = iters = None
    if debug:
        sizes = [(H // 8, W // 8, 64), (H // 4, W // 4, 32), (H // 2, W // 2, 16)]
        feat = torch.empty(sum(n * h * w * c for h, w, c in sizes), dtype=_F32, device=dev)
        iters = torch.empty(sum(n * h * w * k for (h, w, _), k in zip(sizes, (2, 2, 1))), dtype=_F32, device=dev)
    ws = _take_workspace(L.gtsfm_patchmatchnet_workspace_bytes(n, S, H, W), dev, workspace, stream,
                         f"gtsfm_patchmatchnet_batched: unsupported shape {n} views with {S} sources of {H} x {W}")
    rc = L.gtsfm_patchmatchnet_batched(_ptr(images), n, H, W, _ptr(wRc), _ptr(wtc), _ptr(intrinsics), _ptr(src_views),
                                       S, _ptr(depth_range), _ptr(weights), _ptr(init_uniform),
                                       None if config is None else ctypes.addressof(config), _ptr(ws), ws.numel(),
                                       _ptr(r.depth), _ptr(r.confidence), _ptr(feat), _ptr(iters),
                                       native.stream_handle(stream))
    native.check(rc, "gtsfm_patchmatchnet_batched")
    if debug:
        r.features = tuple(t.view(n, h, w, c) for t, (h, w, c) in
                           zip(feat.split([n * h * w * c for h, w, c in sizes]), sizes))
        maps = [s for s, k in zip(sizes, (2, 2, 1)) for _ in range(k)]
        r.iter_depths = tuple(t.view(n, h, w) for t, (h, w, _) in zip(iters.split([n * h * w for h, w, _ in maps]), maps))
    return r
