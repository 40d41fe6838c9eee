"""The reference's track triangulation restated in numpy, independent of the kernels, with its decision margins.

Route restated: gtsfm/data_association/point3d_initializer.py:117-380 (Point3dInitializer.triangulate,
execute_ransac_variant), gtsfm/utils/reprojection.py:48-83, gtsfm/utils/tracks.py:82-102 with
gtsfm/densify/mvs_utils.py:43-50, on GTSAM's triangulatePoint3(rank_tol=1e-9, optimize=True): DLT by np.linalg.svd
(rank >= 3), then Levenberg-Marquardt on the unit-noise reprojection factors (lambda 1, factor 10, <= 100 iterations,
GTSAM's accept rule, absoluteErrorTol 1), cheirality in every camera used. The two stated deviations of
include/gtsfm_hip.h are restated too: the hypothesis set is the m pairs of smallest (key_j, j) (splitmix64 of
(seed, track id, j), or descending squared baseline), and the winner is the minimum of (-votes, avg_err, j).

Everything is batched over hypotheses / tracks (numpy arrays with a leading batch axis and a `use` mask over a padded
measurement axis), so the door fixture's 130k two-view solves take seconds. The linearised cost of an LM step is
summed factor by factor (|J d + e|^2), the kernels use the equivalent quadratic form.

For every track the result carries how close each decision came to flipping (Margins); a track is a near-tie when
one of them is below `delta`: there the deciding quantity is within rounding of its threshold and two correct
implementations may disagree.
"""
import json
import os
from typing import NamedTuple, Optional

import numpy as np

NO_RANSAC, UNIFORM, BIASED, TOPK = 0, 1, 2, 3
SUCCESS, CHEIRALITY, INLIERS_UNDER, POSES_UNDER, EXCEEDS, LOW_ANGLE = range(6)

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DOOR_TRACKS = os.path.join(GOLDEN_DIR, "triangulation", "door_tracks2d.npz")
DOOR_CAMERAS = os.path.join(GOLDEN_DIR, "lund_door", "gt.json")

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


class Cameras(NamedTuple):
    wRc: np.ndarray  # (n_img, 3, 3)
    wtc: np.ndarray  # (n_img, 3)
    intr: np.ndarray  # (n_img, 3) f, u0, v0
    valid: np.ndarray  # (n_img,) bool


class Margins(NamedTuple):
    thresh: np.ndarray  # smallest |err - threshold| over the measurements, under the contending hypotheses + final
    gap: np.ndarray  # avg_err gap between the best and the runner-up hypothesis when their votes are equal, else inf
    z: np.ndarray  # smallest |z| of a measurement's point in its camera frame, same solves
    lm: np.ndarray  # smallest |decrease - 1| the LM loops of those solves saw at their stopping test
    angle: np.ndarray  # |max angle - min_triangulation_angle| (inf when the test is not reached)

    def near_tie(self, delta: float) -> np.ndarray:
        return (self.thresh < delta) | (self.gap < delta) | (self.z < delta) | (self.lm < delta) | (self.angle < delta)


class RefResult(NamedTuple):
    exit_code: np.ndarray  # (T,) int32
    point: np.ndarray  # (T, 3), NaN where the final triangulation did not succeed
    avg_err: np.ndarray  # (T,)
    inlier: np.ndarray  # (n_meas,) uint8
    n_hyp: np.ndarray  # (T,) int32: hypotheses evaluated
    hyp_pair: np.ndarray  # (sum n_hyp,) int64: their pair indices, ascending inside a track
    stats: np.ndarray  # (8,) int64
    margins: Margins
    depth: np.ndarray  # (T,) mean z of the point over the cameras of the final solve (NaN without one)


def load_door():
    """(offsets, image, uv float32, Cameras) of the door fixture with its ground-truth cameras."""
    z = np.load(DOOR_TRACKS)
    with open(DOOR_CAMERAS) as f:
        gt = json.load(f)
    n = len(gt["wRc"])
    cams = Cameras(np.array(gt["wRc"], np.float64).reshape(n, 3, 3), np.array(gt["wtc"], np.float64).reshape(n, 3),
                   np.tile(np.array(gt["fx_u0_v0"], np.float64), (n, 1)), np.ones(n, bool))
    return z["offsets"], z["image"], z["uv"], cams


def circle_cameras() -> Cameras:
    """gtsam.examples.SFMdata.createPoses restated: eight cameras on a circle of radius 40 at height 10, every one
    looking at the origin with world z up (CalibratedCamera::LookatPose: z = target - eye, x = -up x z, y = z x x, all
    normalised), f = 50, principal point 0."""
    R, t = [], []
    up = np.array([0.0, 0.0, 1.0])
    for th in np.linspace(0, 2 * np.pi, 8, endpoint=False):
        eye = np.array([40 * np.cos(th), 40 * np.sin(th), 10.0])
        zc = -eye / np.linalg.norm(eye)
        xc = np.cross(-up, zc)
        xc /= np.linalg.norm(xc)
        yc = np.cross(zc, xc)
        R.append(np.stack([xc, yc, zc], axis=1))
        t.append(eye)
    return Cameras(np.array(R), np.array(t), np.tile(np.array([50.0, 0.0, 0.0]), (8, 1)), np.ones(8, bool))


def project(cams: Cameras, img: np.ndarray, X: np.ndarray):
    """(uv, z) of points X (..., 3) in cameras img (...)."""
    pc = np.einsum("...ji,...j->...i", cams.wRc[img], X - cams.wtc[img])
    with np.errstate(divide="ignore", invalid="ignore"):
        uv = cams.intr[img][..., 1:3] + cams.intr[img][..., :1] * (pc[..., :2] / pc[..., 2:3])
    return uv, pc[..., 2]


def _mix(z: np.ndarray) -> np.ndarray:
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def pair_keys(mode: int, seed: int, track_id: int, img: np.ndarray, cams: Cameras) -> np.ndarray:
    """key_j (uint64) of every pair of a track, combinations order."""
    n = len(img)
    k1, k2 = np.triu_indices(n, 1)
    if mode == UNIFORM:
        tkey = _mix(np.uint64(seed) ^ _mix(np.uint64(track_id & 0xFFFFFFFF if track_id >= 0 else track_id % (1 << 32))))
        with np.errstate(over="ignore"):
            return _mix(tkey + np.arange(len(k1), dtype=np.uint64))
    i1, i2 = img[k1], img[k2]
    ok = _cam_ok(cams, i1) & _cam_ok(cams, i2)
    a, b = cams.wtc[np.where(ok, i1, 0)], cams.wtc[np.where(ok, i2, 0)]
    d = a - b
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    key = ~d2.view(np.uint64)
    return np.where(ok, key, _M64)


def _cam_ok(cams: Cameras, img: np.ndarray) -> np.ndarray:
    img = np.asarray(img)
    inside = (img >= 0) & (img < len(cams.valid))
    return inside & cams.valid[np.where(inside, img, 0)]


def _factors(cams, img, uv, use, p):
    """e (B, n, 2), J (B, n, 2, 3), total 0.5 |e|^2 (B,) of the unit-noise reprojection factors at p (B, 3)."""
    R, f = cams.wRc[img], cams.intr[img][..., 0]
    pr, z = project(cams, img, p[:, None, :])
    pc = np.einsum("bnji,bnj->bni", R, p[:, None, :] - cams.wtc[img])
    front = z > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        iz = 1.0 / pc[..., 2]
        xn, yn = pc[..., 0] * iz, pc[..., 1] * iz
        D = np.zeros(img.shape + (2, 3))
        D[..., 0, 0] = f * iz
        D[..., 0, 2] = -f * xn * iz
        D[..., 1, 1] = f * iz
        D[..., 1, 2] = -f * yn * iz
    J = np.einsum("bnrk,bnjk->bnrj", D, R)
    e = pr - uv
    e = np.where(front[..., None], e, (2.0 * f)[..., None])
    J = np.where(front[..., None, None], J, 0.0)
    e = np.where(use[..., None], e, 0.0)
    J = np.where(use[..., None, None], J, 0.0)
    return e, J, 0.5 * (e * e).sum(axis=(1, 2))


def _chol_solve3(H, g):
    """Batched 3 x 3 Cholesky solve; ok = every pivot > 0."""
    B = len(H)
    L = np.zeros_like(H)
    ok = np.ones(B, bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        for j in range(3):
            s = H[:, j, j] - (L[:, j, :j] ** 2).sum(axis=1)
            ok &= s > 0
            d = np.sqrt(np.where(s > 0, s, 1.0))
            L[:, j, j] = d
            for i in range(j + 1, 3):
                L[:, i, j] = (H[:, i, j] - (L[:, i, :j] * L[:, j, :j]).sum(axis=1)) / d
        y = np.zeros_like(g)
        for i in range(3):
            y[:, i] = (g[:, i] - (L[:, i, :i] * y[:, :i]).sum(axis=1)) / L[:, i, i]
        x = np.zeros_like(g)
        for i in (2, 1, 0):
            x[:, i] = (y[:, i] - (L[:, i + 1:, i] * x[:, i + 1:]).sum(axis=1)) / L[:, i, i]
    return x, ok


def triangulate_batch(cams: Cameras, img: np.ndarray, uv: np.ndarray, use: np.ndarray):
    """triangulatePoint3 of B problems: img (B, n), uv (B, n, 2), use (B, n) (every used camera valid).
    Returns (ok (B,), point (B, 3), lm_margin (B,), min |z| over the used cameras (B,), mean z (B,))."""
    B, n = use.shape
    img = np.where(use, img, 0)
    R, t, K = cams.wRc[img], cams.wtc[img], cams.intr[img]
    Rt = np.swapaxes(R, -1, -2)
    P = np.concatenate([Rt, -np.einsum("bnij,bnj->bni", Rt, t)[..., None]], axis=-1)  # (B, n, 3, 4)
    r0 = uv[..., 0, None] * P[..., 2, :] - (K[..., 0, None] * P[..., 0, :] + K[..., 1, None] * P[..., 2, :])
    r1 = uv[..., 1, None] * P[..., 2, :] - (K[..., 0, None] * P[..., 1, :] + K[..., 2, None] * P[..., 2, :])
    A = np.stack([r0, r1], axis=2) * use[..., None, None]
    A = A.reshape(B, 2 * n, 4)
    if 2 * n < 4:
        A = np.concatenate([A, np.zeros((B, 4 - 2 * n, 4))], axis=1)
    A = np.where(np.isfinite(A), A, 0.0)
    _, s, Vt = np.linalg.svd(A)
    ok = (s > 1e-9).sum(axis=1) >= 3
    v = Vt[:, -1, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        p = v[:, :3] / v[:, 3:4]
    p = np.where(ok[:, None], p, 0.0)
    _, _, err = _factors(cams, img, uv, use, p)
    lam = np.ones(B)
    iters = np.zeros(B, int)
    lm_margin = np.full(B, np.inf)
    active = ok & np.isfinite(err) & (err > 0)
    for _ in range(200):
        idx = np.flatnonzero(active)
        if len(idx) == 0:
            break
        cur = err[idx].copy()
        e, J, _ = _factors(cams, img[idx], uv[idx], use[idx], p[idx])
        H = np.einsum("bnri,bnrj->bij", J, J)
        g = -np.einsum("bnri,bnr->bi", J, e)
        old_lin = 0.5 * (e * e).sum(axis=(1, 2))
        pending = np.ones(len(idx), bool)
        for _inner in range(64):
            q = np.flatnonzero(pending)
            if len(q) == 0:
                break
            gi = idx[q]
            d, chol_ok = _chol_solve3(H[q] + lam[gi, None, None] * np.eye(3), g[q])
            d = np.where(chol_ok[:, None], d, 0.0)
            new_lin = 0.5 * ((np.einsum("bnri,bi->bnr", J[q], d) + e[q]) ** 2).sum(axis=(1, 2))
            lin_change = old_lin[q] - new_lin
            cond = chol_ok & (lin_change >= 0)
            new_p = p[gi] + d
            _, _, new_err = _factors(cams, img[gi], uv[gi], use[gi], new_p)
            cost_change = err[gi] - new_err
            with np.errstate(divide="ignore", invalid="ignore"):
                good_ratio = cost_change / lin_change > 1e-3
            success = cond & np.where(lin_change > np.finfo(float).eps * old_lin[q], good_ratio, True)
            stop = cond & (np.abs(cost_change) < 1e-5 * err[gi])
            s_i = gi[success]
            p[s_i], err[s_i] = new_p[success], new_err[success]
            lam[s_i] /= 10.0
            iters[s_i] += 1
            grow = ~success & ~stop
            lam[gi[grow]] *= 10.0
            pending[q[success | stop | (grow & (lam[gi] >= 1e5))]] = False
        dec = cur - err[idx]
        lm_margin[idx] = np.minimum(lm_margin[idx], np.abs(dec - 1.0))
        with np.errstate(divide="ignore", invalid="ignore"):
            done = (iters[idx] >= 100) | (dec / cur <= 1e-5) | (dec <= 1.0) | ~np.isfinite(cur)
        active[idx[done]] = False
    _, z = project(cams, img, p[:, None, :])
    zu = np.where(use, z, np.inf)
    ok = ok & (zu > 0).all(axis=1)
    with np.errstate(invalid="ignore"):
        zmean = np.where(use, z, 0.0).sum(axis=1) / np.maximum(use.sum(axis=1), 1)
    return ok, p, lm_margin, np.abs(zu).min(axis=1), zmean


def reproj_errors(cams: Cameras, img: np.ndarray, uv: np.ndarray, present: np.ndarray, X: np.ndarray):
    """err (B, n) of measurements against X (B, 3): NaN for an invalid camera or z <= 0 (absent slots too), and z."""
    okc = _cam_ok(cams, img) & present
    im = np.where(okc, img, 0)
    pr, z = project(cams, im, X[:, None, :])
    with np.errstate(invalid="ignore"):
        err = np.sqrt(((uv - pr) ** 2).sum(axis=-1))
    return np.where(okc & (z > 0), err, np.nan), np.where(okc, z, np.inf)


def select_pairs(mode, seed, track_id, img, cams, n_hyp) -> np.ndarray:
    n = len(img)
    n_pairs = n * (n - 1) // 2
    m = min(n_hyp, n_pairs)
    if m == n_pairs:
        return np.arange(n_pairs, dtype=np.int64)
    keys = pair_keys(mode, seed, track_id, img, cams)
    order = np.lexsort((np.arange(n_pairs), keys))
    return np.sort(order[:m]).astype(np.int64)


def triangulate_tracks(offsets, image, uv, cams: Cameras, mode: int, thresh: float, min_angle: float = 0.0,
                       n_hyp: int = 0, seed: int = 0, track_id: Optional[np.ndarray] = None) -> RefResult:
    offsets = np.asarray(offsets, np.int64)
    image = np.asarray(image, np.int64)
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    T = len(offsets) - 1
    lens = np.diff(offsets)
    nmax = max(int(lens.max()) if T else 0, 2)
    # padded per-track arrays
    slot = np.arange(nmax)[None, :]
    present = slot < lens[:, None]
    pos = np.where(present, offsets[:-1, None] + slot, 0)
    t_img = np.where(present, image[pos] if len(image) else 0, -1)
    t_uv = np.where(present[..., None], uv[pos] if len(uv) else 0.0, 0.0)
    inf = np.full(T, np.inf)
    m_thresh, m_gap, m_z, m_lm, m_angle = inf.copy(), inf.copy(), inf.copy(), inf.copy(), inf.copy()
    best = np.zeros((T, nmax), bool)
    n_hyp_t = np.zeros(T, np.int32)
    hyp_pair = np.zeros(0, np.int64)
    if mode == NO_RANSAC:
        best = present.copy()
    else:
        h_track, h_j, h_k1, h_k2 = [], [], [], []
        for t in range(T):
            n = int(lens[t])
            if n < 2:
                continue
            js = select_pairs(mode, seed, int(track_id[t]) if track_id is not None else t, t_img[t, :n], cams, n_hyp)
            k1, k2 = np.triu_indices(n, 1)
            h_track.append(np.full(len(js), t))
            h_j.append(js)
            h_k1.append(k1[js])
            h_k2.append(k2[js])
            n_hyp_t[t] = len(js)
        if h_track:
            h_track, h_j = np.concatenate(h_track), np.concatenate(h_j)
            h_k1, h_k2 = np.concatenate(h_k1), np.concatenate(h_k2)
            hyp_pair = h_j
            kk = np.stack([h_k1, h_k2], axis=1)
            h_img = t_img[h_track[:, None], kk]
            h_uv = t_uv[h_track[:, None], kk]
            cam_ok = _cam_ok(cams, h_img).all(axis=1)
            ok, X, lm, zmin, _ = triangulate_batch(cams, np.where(cam_ok[:, None], h_img, 0), h_uv,
                                                   np.repeat(cam_ok[:, None], 2, axis=1))
            ok &= cam_ok
            err, z = reproj_errors(cams, t_img[h_track], t_uv[h_track], present[h_track], np.where(ok[:, None], X, 0.0))
            with np.errstate(invalid="ignore"):
                inl = ok[:, None] & (err < thresh)
            votes = inl.sum(axis=1)
            with np.errstate(invalid="ignore", divide="ignore"):
                avg = np.where(inl, err, 0.0).sum(axis=1) / votes
            # per-hypothesis margins (a skipped hypothesis has none of its own: its failure is a z / rank decision)
            with np.errstate(invalid="ignore"):
                h_thr = np.nanmin(np.where(np.isnan(err), np.inf, np.abs(err - thresh)), axis=1)
            h_z = np.minimum(np.where(ok, np.abs(z).min(axis=1), np.inf), zmin)  # a failed solve: its own cameras only
            h_thr = np.where(cam_ok, h_thr, np.inf)
            h_z = np.where(cam_ok, h_z, np.inf)
            h_lm = np.where(cam_ok, lm, np.inf)
            order = np.lexsort((h_j, np.where(votes > 0, avg, np.inf), -votes, h_track))
            starts = np.flatnonzero(np.concatenate([[True], h_track[order][1:] != h_track[order][:-1]]))
            ends = np.concatenate([starts[1:], [len(order)]])
            for s, e in zip(starts, ends):
                o = order[s:e]
                t = h_track[o[0]]
                b = o[0]
                # every hypothesis that is one vote from the best contends; a failed one contends through z only
                cont = o[(votes[o] >= votes[b] - 1)]
                m_thresh[t] = min(m_thresh[t], h_thr[cont].min())
                m_z[t] = min(m_z[t], h_z[o].min())
                m_lm[t] = min(m_lm[t], h_lm[cont].min())
                if votes[b] > 0:
                    best[t] = inl[b]
                    if len(o) > 1 and votes[o[1]] == votes[b]:
                        m_gap[t] = abs(avg[o[1]] - avg[b])
    inlier = np.zeros(len(image), np.uint8)
    inlier[(offsets[:-1, None] + slot)[present]] = best[present]
    n_inl = best.sum(axis=1)
    posed = best & _cam_ok(cams, t_img)
    n_posed = posed.sum(axis=1)
    exit_code = np.full(T, -1, np.int32)
    exit_code[n_inl < 2] = INLIERS_UNDER
    exit_code[(exit_code < 0) & (n_posed < 2)] = POSES_UNDER
    point = np.full((T, 3), np.nan)
    avg_err = np.full(T, np.nan)
    depth = np.full(T, np.nan)
    go = np.flatnonzero(exit_code < 0)
    if len(go):
        ok, X, lm, zmin, zmean = triangulate_batch(cams, np.where(posed[go], t_img[go], 0), t_uv[go], posed[go])
        m_lm[go] = np.minimum(m_lm[go], lm)
        m_z[go] = np.minimum(m_z[go], zmin)
        exit_code[go[~ok]] = CHEIRALITY
        g2, X2 = go[ok], X[ok]
        point[g2] = X2
        depth[g2] = zmean[ok]
        err, z = reproj_errors(cams, t_img[g2], t_uv[g2], best[g2], X2)
        with np.errstate(invalid="ignore"):
            m_thresh[g2] = np.minimum(m_thresh[g2], np.where(np.isnan(err), np.inf, np.abs(err - thresh)).min(axis=1))
            m_z[g2] = np.minimum(m_z[g2], np.abs(z).min(axis=1))
            fin = ~np.isnan(err)
            avg_err[g2] = np.where(fin.any(axis=1), np.where(fin, err, 0.0).sum(axis=1) / np.maximum(fin.sum(axis=1), 1),
                                   np.nan)
            all_in = (np.where(best[g2], err < thresh, True)).all(axis=1)
        exit_code[g2[~all_in]] = EXCEEDS
        g3 = g2[all_in]
        exit_code[g3] = SUCCESS
        if min_angle > 0 and len(g3):
            rays = point[g3][:, None, :] - cams.wtc[np.where(best[g3], t_img[g3], 0)]
            rays = rays / np.sqrt((rays * rays).sum(axis=-1, keepdims=True))
            dots = np.clip(np.einsum("tai,tbi->tab", rays, rays), -1.0, 1.0)
            pair_ok = best[g3][:, :, None] & best[g3][:, None, :] & ~np.eye(nmax, dtype=bool)[None]
            min_dot = np.where(pair_ok, dots, np.inf).min(axis=(1, 2))
            angle = np.rad2deg(np.arccos(min_dot))
            m_angle[g3] = np.abs(angle - min_angle)
            exit_code[g3[angle < min_angle]] = LOW_ANGLE
    stats = np.zeros(8, np.int64)
    stats[:6] = np.bincount(exit_code, minlength=6)[:6]
    stats[6] = n_inl[exit_code == SUCCESS].sum()
    stats[7] = n_hyp_t.sum()
    return RefResult(exit_code, point, avg_err, inlier, n_hyp_t, hyp_pair, stats,
                     Margins(m_thresh, m_gap, m_z, m_lm, m_angle), depth)


def reverse_measurements(offsets, image, uv):
    """The same tracks with every track's measurements in reversed order."""
    offsets = np.asarray(offsets, np.int64)
    idx = np.concatenate([np.arange(offsets[t + 1] - 1, offsets[t] - 1, -1) for t in range(len(offsets) - 1)]
                         or [np.zeros(0, np.int64)])
    return np.asarray(image)[idx], np.asarray(uv)[idx], idx


def lookat_cameras(eyes: np.ndarray, f: float = 800.0, pp=(500.0, 400.0)) -> Cameras:
    """Cameras at `eyes` (n, 3) looking at the origin, world z up (LookatPose)."""
    R = []
    up = np.array([0.0, 0.0, 1.0])
    for eye in eyes:
        zc = -eye / np.linalg.norm(eye)
        xc = np.cross(-up, zc)
        xc /= np.linalg.norm(xc)
        R.append(np.stack([xc, np.cross(zc, xc), zc], axis=1))
    n = len(eyes)
    return Cameras(np.array(R), np.asarray(eyes, np.float64), np.tile(np.array([f, pp[0], pp[1]]), (n, 1)),
                   np.ones(n, bool))


def make_synth(n_cam: int = 40, n_tracks: int = 300, seed: int = 0, outlier_share: float = 0.2, noise: float = 0.5):
    """A seeded scene for the selection path: n_cam cameras on a ring of radius 10 (heights vary) around points in a
    ball of radius 2; track lengths cycle through 2, 3, 15, 16, n_cam and a few random ones; a share of the
    measurements is moved by 50-150 px (gross outliers), the rest get Gaussian noise. uv is float64.
    Returns (offsets, image, uv, cams, is_outlier)."""
    rng = np.random.default_rng(seed)
    th = np.linspace(0, 2 * np.pi, n_cam, endpoint=False)
    eyes = np.stack([10 * np.cos(th), 10 * np.sin(th), rng.uniform(-1.5, 1.5, n_cam)], axis=1)
    cams = lookat_cameras(eyes)
    fixed = [2, 3, 15, 16, n_cam]
    lens = [fixed[t % 5] if t < 25 else int(rng.integers(2, 13)) for t in range(n_tracks)]
    offsets = np.zeros(n_tracks + 1, np.int32)
    np.cumsum(lens, out=offsets[1:])
    image, uv, outl = [], [], []
    for t in range(n_tracks):
        X = rng.normal(size=3)
        X = X / np.linalg.norm(X) * rng.uniform(0, 2)
        cam_ids = np.sort(rng.choice(n_cam, lens[t], replace=False))
        p, _ = project(cams, cam_ids, np.tile(X, (lens[t], 1)))
        bad = rng.random(lens[t]) < outlier_share
        ang = rng.uniform(0, 2 * np.pi, lens[t])
        shift = rng.uniform(50, 150, lens[t])[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1)
        p = p + np.where(bad[:, None], shift, rng.normal(scale=noise, size=(lens[t], 2)))
        image.append(cam_ids)
        uv.append(p)
        outl.append(bad)
    return (offsets, np.concatenate(image).astype(np.int32), np.concatenate(uv), cams, np.concatenate(outl))


def rounding_floor(delta: float = 1e-6):
    """The restatement's own rounding floor on the door fixture (NO_RANSAC, threshold 1e5): the same tracks with every
    track's measurements reversed are the same problems in another summation order. Returns the maxima over the
    tracks that are no near-tie of |dX| / depth and of |d avg_err|."""
    off, img, uv, cams = load_door()
    a = triangulate_tracks(off, img, uv, cams, NO_RANSAC, 1e5)
    img_r, uv_r, _ = reverse_measurements(off, img, uv)
    b = triangulate_tracks(off, img_r, uv_r, cams, NO_RANSAC, 1e5)
    keep = ~a.margins.near_tie(delta) & ~b.margins.near_tie(delta) & np.isfinite(a.point).all(axis=1)
    assert np.array_equal(a.exit_code[keep], b.exit_code[keep])
    dx = np.linalg.norm(a.point - b.point, axis=1)[keep] / a.depth[keep]
    de = np.abs(a.avg_err - b.avg_err)[keep]
    return float(dx.max()), float(de.max())
