"""float64 numpy restatement of the dense-MVS geometry calls (gtsfm_mvs_*, semantics in include/gtsfm_hip.h), with the
float32 roundings at the same points, and the analytic scene the MVS tests run on.

Written from the header, not from the reference's code. cv2, open3d and gtsam are not available to the test suite, so
the reference's own code cannot be run to produce goldens: this restatement is instead pinned to hand-derived answers
by tests/test_mvs.py (closed-form angles and Gaussians, np.percentile, a fronto-parallel plane seen by two translated
cameras, the colour rule for all 256 values, a brute-force voxel dictionary).
"""
import functools
from typing import NamedTuple, Optional

import numpy as np

SCORE_SCALE = 2.0 ** 40
ERR_SCALE = 2.0 ** 24
F32 = np.float32


# ---------------------------------------------------------------------------------------------- view selection
def piecewise_gaussian(theta, theta_0=5.0, sigma_1=1.0, sigma_2=10.0):
    theta = np.asarray(theta, np.float64)
    sigma = np.where(theta <= theta_0, sigma_1, sigma_2)
    return np.exp(-((theta - theta_0) ** 2) / (2.0 * sigma * sigma))


def triangulation_angle_deg(c1, c2, X):
    r1, r2 = np.asarray(X, np.float64) - c1, np.asarray(X, np.float64) - c2
    r1 = r1 / np.sqrt((r1 * r1).sum(-1, keepdims=True))
    r2 = r2 / np.sqrt((r2 * r2).sum(-1, keepdims=True))
    return np.arccos(np.clip((r1 * r2).sum(-1), -1.0, 1.0)) * 57.29577951308232


def percentile(values, q):
    """np.percentile(values, 100 q), method 'linear', spelt out: virtual index (n - 1) q and numpy's two-sided lerp."""
    v = np.sort(np.asarray(values, np.float64))
    n = len(v)
    pos = (n - 1) * q
    lo = int(np.floor(pos))
    hi = min(lo + 1, n - 1)
    t = pos - lo
    a, b = v[lo], v[hi]
    return b - (b - a) * (1.0 - t) if t >= 0.5 else a + (b - a) * t


class ViewsRef(NamedTuple):
    img_to_pm: np.ndarray
    pm_to_img: np.ndarray    # (n_valid,)
    scores: np.ndarray       # (n_valid, n_valid) int64, units of 2^-40
    scores_float: np.ndarray  # the same sums in float64
    terms: np.ndarray        # (n_valid, n_valid) terms added per entry
    src_views: np.ndarray    # (n_valid, V - 1)
    depth_range: np.ndarray  # (n_valid, 2)
    stats: np.ndarray


def source_views(scores: np.ndarray, max_num_views: int) -> np.ndarray:
    """Row r: the V - 1 other views of highest score, descending, ties to the lower index."""
    nv = scores.shape[0]
    picks = max(min(max_num_views, nv) - 1, 0)
    out = np.zeros((nv, picks), np.int32)
    for r in range(nv):
        others = [c for c in range(nv) if c != r]
        others.sort(key=lambda c: (-int(scores[r, c]), c))
        out[r] = others[:picks]
    return out


def select_views(offsets, img, point, track_keep, inlier, wRc, wtc, cam_keep, max_num_views=5) -> ViewsRef:
    n_img = len(wtc)
    keep = np.ones(n_img, bool) if cam_keep is None else np.asarray(cam_keep) != 0
    pm_to_img = np.flatnonzero(keep).astype(np.int32)
    nv = len(pm_to_img)
    img_to_pm = np.full(n_img, -1, np.int32)
    img_to_pm[pm_to_img] = np.arange(nv)
    scores = np.zeros((nv, nv), np.int64)
    scores_f = np.zeros((nv, nv))
    terms = np.zeros((nv, nv), np.int64)
    depths = [[] for _ in range(nv)]
    for t in range(len(offsets) - 1):
        if track_keep is not None and not track_keep[t]:
            continue
        ms = [m for m in range(offsets[t], offsets[t + 1])
              if (inlier is None or inlier[m]) and 0 <= img[m] < n_img and img_to_pm[img[m]] >= 0]
        for k1, m1 in enumerate(ms):
            c1 = img[m1]
            depths[img_to_pm[c1]].append(float(wRc[c1][:, 2] @ (point[t] - wtc[c1])))
            for m2 in ms[k1 + 1:]:
                c2 = img[m2]
                a, b = img_to_pm[c1], img_to_pm[c2]
                if a == b:
                    continue
                s = float(piecewise_gaussian(triangulation_angle_deg(wtc[c1], wtc[c2], point[t])))
                if not 0.0 <= s <= 1.0:
                    continue
                q = int(np.floor(s * SCORE_SCALE + 0.5))
                for x, y in ((a, b), (b, a)):
                    scores[x, y] += q
                    scores_f[x, y] += s
                    terms[x, y] += 1
    rng = np.full((nv, 2), np.nan)
    for r in range(nv):
        if depths[r]:
            rng[r] = percentile(depths[r], 0.01), percentile(depths[r], 0.99)
    stats = np.array([nv, max(min(max_num_views, nv) - 1, 0), sum(1 for d in depths if not d), terms.sum() // 2],
                     np.int64)
    return ViewsRef(img_to_pm, pm_to_img, scores, scores_f, terms, source_views(scores, max_num_views), rng, stats)


# ---------------------------------------------------------------------------------------------- fusion
def _transfer(Ra, ta, Ka, Rb, tb, u, v, d):
    """Pixel (u, v) at depth d of camera a in the frame of camera b, in the kernel's order of operations."""
    xc, yc = (u - Ka[1]) / Ka[0] * d, (v - Ka[2]) / Ka[0] * d
    w = [(Ra[i, 0] * xc + Ra[i, 1] * yc + Ra[i, 2] * d + ta[i]) - tb[i] for i in range(3)]
    return [Rb[0, j] * w[0] + Rb[1, j] * w[1] + Rb[2, j] * w[2] for j in range(3)]


def bilinear_zero_border(m: np.ndarray, x: np.ndarray, y: np.ndarray) -> np.ndarray:
    """float32 bilinear sample of map m (H, W) at float32 (x, y), taps outside the map = 0."""
    H, W = m.shape
    inside = (x > -1) & (x < W) & (y > -1) & (y < H)
    xs, ys = np.where(inside, x, F32(0)), np.where(inside, y, F32(0))
    fx, fy = np.floor(xs), np.floor(ys)
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    ax, ay = (xs - fx).astype(F32), (ys - fy).astype(F32)

    def tap(yy, xx):
        ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        return np.where(ok, m[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], F32(0)).astype(F32)

    bx, by = F32(1) - ax, F32(1) - ay
    with np.errstate(invalid="ignore"):
        s = ((tap(y0, x0) * bx) * by + (tap(y0, x0 + 1) * ax) * by) + ((tap(y0 + 1, x0) * bx) * ay
                                                                        + (tap(y0 + 1, x0 + 1) * ax) * ay)
    return np.where(inside, s, F32(0)).astype(F32)


def reproject(depth, wRc, wtc, intr, r, s):
    """dist (float64), rel (float32), d_reproj (float32) and the float32 source coordinates of every pixel of view r
    against source s."""
    H, W = depth.shape[1:]
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    d_ref = depth[r].astype(F32)
    with np.errstate(all="ignore"):
        xs = _transfer(wRc[r], wtc[r], intr[r], wRc[s], wtc[s], x, y, d_ref.astype(np.float64))
        us, vs = intr[s][0] * xs[0] / xs[2] + intr[s][1], intr[s][0] * xs[1] / xs[2] + intr[s][2]
        usf, vsf = us.astype(F32), vs.astype(F32)
        sampled = bilinear_zero_border(depth[s].astype(F32), usf, vsf)
        xr = _transfer(wRc[s], wtc[s], intr[s], wRc[r], wtc[r], us, vs, sampled.astype(np.float64))
        d_rep = xr[2].astype(F32)
        ur = (intr[r][0] * xr[0] / xr[2] + intr[r][1]).astype(F32)
        vr = (intr[r][0] * xr[1] / xr[2] + intr[r][2]).astype(F32)
        dx, dy = ur.astype(np.float64) - x, vr.astype(np.float64) - y
        dist = np.sqrt(dx * dx + dy * dy)
        rel = (np.abs(d_rep - d_ref) / d_ref).astype(F32)
    ok = np.isfinite(d_ref) & (d_ref > 0)
    dist = np.where(ok, dist, np.nan)
    return dist, rel, d_rep, usf, vsf


class FusedRef(NamedTuple):
    fused: np.ndarray   # (n, H, W) float32
    mask: np.ndarray    # (n, H, W) uint8: 1 geo, 2 conf, 4 joint
    counts: np.ndarray  # (n, 4) int64
    err: np.ndarray     # (n, 3) float64: sum (2^-24 fixed point), min, max
    dist: np.ndarray    # (n, S, H, W) float64, NaN where the reference depth is unusable or the source is none
    rel: np.ndarray     # (n, S, H, W) float32


def fuse_depth(depth, conf, wRc, wtc, intr, src_views, pixel_thresh=1.0, depth_thresh=0.01, min_conf=0.8,
               min_views=1) -> FusedRef:
    n, H, W = depth.shape
    S = src_views.shape[1]
    fused = np.zeros((n, H, W), F32)
    mask = np.zeros((n, H, W), np.uint8)
    counts = np.zeros((n, 4), np.int64)
    err = np.zeros((n, 3))
    dist_all = np.full((n, S, H, W), np.nan)
    rel_all = np.full((n, S, H, W), np.nan, F32)
    for r in range(n):
        geo_sum = np.zeros((H, W), np.int64)
        dsum = np.zeros((H, W), F32)
        near_all = []
        for k in range(S):
            s = int(src_views[r, k])
            if not 0 <= s < n:
                near_all.append(np.zeros((H, W), bool))
                continue
            dist, rel, d_rep, _, _ = reproject(depth, wRc, wtc, intr, r, s)
            dist_all[r, k], rel_all[r, k] = dist, rel
            with np.errstate(invalid="ignore"):
                near = dist < pixel_thresh
                good = near & (rel < F32(depth_thresh))
            geo_sum += good
            dsum = np.where(good, dsum + d_rep, dsum).astype(F32)
            near_all.append(near)
        d_ref = depth[r].astype(F32)
        with np.errstate(invalid="ignore"):
            avg = ((dsum + d_ref).astype(F32).astype(np.float64) / (geo_sum + 1)).astype(F32)
            # A pixel whose own depth is NaN, infinite, 0 or negative is never geometric, whatever min_views is. With
            # min_views >= 1 that follows from geo_sum = 0; with min_views <= 0 the reference's filter would pass it on
            # with (0 + d_ref) / 1 as its fused depth, and a NaN point would reach the cloud.
            geo = (geo_sum >= min_views) & np.isfinite(d_ref) & (d_ref > 0)
            cok = conf[r].astype(F32) > F32(min_conf)
        joint = geo & cok
        fused[r] = np.where(joint, avg, F32(0))
        mask[r] = geo * 1 + cok * 2 + joint * 4
        e = np.concatenate([dist_all[r, k][joint & near_all[k]] for k in range(S)]) if S else np.zeros(0)
        counts[r] = geo.sum(), cok.sum(), joint.sum(), len(e)
        if len(e):
            err[r] = np.floor(e * ERR_SCALE + 0.5).sum() / ERR_SCALE, e.min(), e.max()
    return FusedRef(fused, mask, counts, err, dist_all, rel_all)


def color_rule(c: np.ndarray) -> np.ndarray:
    """The reference's ((float32(c) / 255) * 255).astype(uint8), in float32."""
    return ((np.asarray(c).astype(F32) / F32(255)) * F32(255)).astype(np.uint8)


def gather_points(fused, mask, wRc, wtc, intr, images, view_image=None):
    """points (N, 3), colors (N, 3), view_offset (n + 1,): views ascending, then row-major. The maps cover the
    top-left corner of the images; a view whose image index is outside [0, len(images)) is black."""
    n, H, W = fused.shape
    pts, cols, off = [], [], [0]
    for r in range(n):
        on = (mask[r] & 4) != 0
        yy, xx = np.nonzero(on)  # row-major
        d = fused[r][on].astype(np.float64)
        xc, yc = (xx - intr[r][1]) / intr[r][0] * d, (yy - intr[r][2]) / intr[r][0] * d
        R, t = wRc[r], wtc[r]
        pts.append(np.stack([R[i, 0] * xc + R[i, 1] * yc + R[i, 2] * d + t[i] for i in range(3)], 1))
        im = r if view_image is None else int(view_image[r])
        cols.append(color_rule(images[im][yy, xx]) if 0 <= im < len(images) else np.zeros((len(d), 3), np.uint8))
        off.append(off[-1] + len(d))
    return np.concatenate(pts), np.concatenate(cols), np.array(off, np.int64)


# ---------------------------------------------------------------------------------------------- voxels
def voxel_stats(points: np.ndarray) -> np.ndarray:
    """(18,): mean, scatter / (N - 1), min bound, max bound."""
    out = np.zeros(18)
    n = len(points)
    if n == 0:
        return out
    mean = points.sum(0) / n
    c = points - mean
    out[0:3] = mean
    if n >= 2:
        out[3:12] = (c.T @ c / (n - 1)).reshape(9)
    out[12:15], out[15:18] = points.min(0), points.max(0)
    return out


def voxel_size(stats: np.ndarray, n: int, scale: float = 0.02) -> float:
    if n < 2:
        return 0.0
    return scale * float(np.sqrt(max(np.linalg.eigvalsh(stats[3:12].reshape(3, 3))[0], 0.0)))


def voxel_keys(points, min_bound, voxel):
    idx = np.floor((points - (min_bound - voxel / 2.0)) / voxel)
    idx = np.clip(idx, 0, 2 ** 21 - 1).astype(np.int64)
    return (idx[:, 0] << 42) | (idx[:, 1] << 21) | idx[:, 2]


def voxel_downsample(points, colors, min_bound, voxel):
    """(points, colors, keys, counts) in ascending key order; colours are the truncated integer mean."""
    keys = voxel_keys(points, min_bound, voxel)
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    heads = np.flatnonzero(np.r_[True, sk[1:] != sk[:-1]])
    ends = np.r_[heads[1:], len(sk)]
    out_p = np.zeros((len(heads), 3))
    out_c = np.zeros((len(heads), 3), np.uint8)
    for j, (lo, hi) in enumerate(zip(heads, ends)):
        s = np.zeros(3)
        for q in order[lo:hi]:  # the kernel's order: ascending input index within a voxel
            s = s + points[q]
        out_p[j] = s / (hi - lo)
        out_c[j] = colors[order[lo:hi]].astype(np.int64).sum(0) // (hi - lo)
    return out_p, out_c, sk[heads], (ends - heads).astype(np.int32)


# ---------------------------------------------------------------------------------------------- the scene
PLANE_Z = 10.0                                  # the plane z = PLANE_Z of the world, seen from cameras near z = 0
SPHERE_C, SPHERE_R = np.array([0.3, -0.2, 7.0]), 1.5
FOCAL_PER_WIDTH = 1.1


def look_at(center, target, up=np.array([0.0, -1.0, 0.0])):
    """Camera-to-world rotation, camera z forward, y down (world y points down as well)."""
    z = target - center
    z = z / np.linalg.norm(z)
    x = np.cross(-up, z)
    x = x / np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z], 1)


def render_depth(wRc, wtc, intr, H, W):
    """Analytic z-depth of the plane and the sphere in front of it at the integer pixel coordinates."""
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    out = np.zeros((len(wtc), H, W))
    for i in range(len(wtc)):
        rays = np.stack([(x - intr[i][1]) / intr[i][0], (y - intr[i][2]) / intr[i][0], np.ones_like(x)], -1) @ wRc[i].T
        o = wtc[i]
        t_plane = (PLANE_Z - o[2]) / rays[..., 2]
        oc = o - SPHERE_C
        a = (rays * rays).sum(-1)
        b = 2.0 * (rays @ oc)
        disc = b * b - 4.0 * a * (oc @ oc - SPHERE_R ** 2)
        t_sphere = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0.0))) / (2.0 * a), np.inf)
        t_sphere = np.where(t_sphere > 0, t_sphere, np.inf)
        out[i] = np.minimum(t_plane, t_sphere)  # rays have camera z = 1: t is the z-depth
    return out


class Scene(NamedTuple):
    wRc: np.ndarray       # per image
    wtc: np.ndarray
    intr: np.ndarray
    cam_keep: np.ndarray
    offsets: np.ndarray   # the tracks
    img: np.ndarray
    point: np.ndarray
    track_keep: np.ndarray
    inlier: np.ndarray
    H: int
    W: int
    depth: np.ndarray     # (n_valid, H, W) float32, per pm_i, corrupted
    conf: np.ndarray
    images: np.ndarray    # (n_img, H, W, 3) uint8
    clean: np.ndarray     # the uncorrupted depth, float64
    dead_view: int        # pm_i of the view whose confidence is all below the threshold


@functools.lru_cache(maxsize=None)
def make_scene(W: int = 72, H: int = 40, seed: int = 11, n_img: int = 7, dropped: Optional[int] = 3,
               focal_spread: float = 0.0, centre_shift: float = 0.0, wrong_fraction: float = 0.05) -> Scene:
    """Cameras on an arc in front of the plane, all looking at the sphere; image `dropped` has cam_keep 0 and sits in
    the middle, so image index != pm_i after it. The last camera looks far to the side: many of its samples, and of
    the samples into it, fall outside the maps. ~300 tracks on the surface with 2-5 measurements each.

    focal_spread and centre_shift make the cameras unequal (the default tiles one (f, cx, cy) over all of them): image i
    has f (1 + focal_spread cos(1.7 i + 0.3)) and its principal point moved by centre_shift (sin(2.1 i + 1),
    0.6 cos(1.3 i + 2)) pixels, an irregular sequence with no symmetry about the middle camera. They draw nothing from
    the generator, so everything else the scene draws stays as it is. wrong_fraction is the share of corrupted
    depths."""
    rng = np.random.default_rng(seed)
    ang = np.linspace(-0.35, 0.35, n_img)
    centres = np.stack([6.0 * np.sin(ang), 0.3 * np.cos(3 * ang), 7.0 - 7.0 * np.cos(ang)], 1)
    targets = np.tile(SPHERE_C, (n_img, 1)) + rng.normal(0, 0.1, (n_img, 3))
    targets[-1] += np.array([3.5, 0.0, 0.0])
    wRc = np.stack([look_at(c, t) for c, t in zip(centres, targets)])
    intr = np.tile(np.array([FOCAL_PER_WIDTH * W, (W - 1) / 2.0, (H - 1) / 2.0]), (n_img, 1))
    if focal_spread or centre_shift:
        i = np.arange(n_img)
        intr[:, 0] *= 1.0 + focal_spread * np.cos(1.7 * i + 0.3)
        intr[:, 1] += centre_shift * np.sin(2.1 * i + 1.0)
        intr[:, 2] += centre_shift * 0.6 * np.cos(1.3 * i + 2.0)
    cam_keep = np.ones(n_img, np.uint8)
    if dropped is not None:
        cam_keep[dropped] = 0
    valid = np.flatnonzero(cam_keep)
    clean_all = render_depth(wRc, centres, intr, H, W)
    # tracks: surface points back-projected from random pixels of random cameras, seen by 2-5 cameras
    offsets, img, pts = [0], [], []
    while len(pts) < 300:
        c = int(rng.integers(n_img))
        px, py = rng.uniform(0, W - 1), rng.uniform(0, H - 1)
        ray = wRc[c] @ np.array([(px - intr[c][1]) / intr[c][0], (py - intr[c][2]) / intr[c][0], 1.0])
        d = render_depth(wRc[c:c + 1], centres[c:c + 1], np.array([[intr[c][0], intr[c][1] - px, intr[c][2] - py]]),
                         1, 1)[0, 0, 0]
        X = centres[c] + d * ray
        k = int(rng.integers(2, 6))
        cams = sorted(rng.choice(n_img, size=min(k, n_img), replace=False).tolist())
        img += cams
        offsets.append(len(img))
        pts.append(X)
    T = len(pts)
    track_keep = (rng.random(T) < 0.9).astype(np.uint8)
    inlier = (rng.random(len(img)) < 0.9).astype(np.uint8)
    # maps per pm_i
    depth = clean_all[valid].astype(F32)
    n = len(valid)
    wrong = rng.random((n, H, W)) < wrong_fraction
    depth = np.where(wrong, depth * rng.uniform(0.5, 1.5, (n, H, W)).astype(F32), depth).astype(F32)
    for r in range(n):
        for value in (0.0, np.nan, -1.0):
            for _ in range(3):
                depth[r, rng.integers(H), rng.integers(W)] = value
    conf = rng.uniform(0.6, 1.0, (n, H, W)).astype(F32)
    conf[:, 0, :4] = F32(0.8)  # exactly at the threshold: not confident
    dead = n - 2
    conf[dead] = rng.uniform(0.1, 0.79, (H, W)).astype(F32)
    images = rng.integers(0, 256, (n_img, H, W, 3)).astype(np.uint8)
    return Scene(wRc, centres, intr, cam_keep, np.array(offsets, np.int32), np.array(img, np.int32), np.array(pts),
                 track_keep, inlier, H, W, depth, conf, images, clean_all[valid], dead)


# The scene with unequal cameras: f varies by +-15 %, the principal points move by up to 5 and 3 pixels. The share of
# wrong depths is 2 %, not 5 %: every wrong depth next to a sample puts a pixel's dist or rel somewhere arbitrary, the
# tighter thresholds of FUSION_PARAMS["tight"] double the density of such values near the threshold, and at 5 % the
# restatement's band of that set covers 1.3 % of a view (measured on the restatement alone; tests/test_mvs.py asserts
# the 1 % cap for every set).
UNEQUAL = dict(focal_spread=0.15, centre_shift=5.0, wrong_fraction=0.02)
FUSION_PARAMS = {"default": {}, "two_views": dict(min_views=2), "three_views": dict(min_views=3),
                 "tight": dict(pixel_thresh=0.5, depth_thresh=0.005, min_conf=0.9), "zero_views": dict(min_views=0)}
# src_views for six views: gaps, no source at all, an entry equal to n_views, one source twice, entries far outside
RAGGED_SRC = np.array([[2, -1, 4, -1], [-1, -1, -1, -1], [0, 6, 3, 1], [1, 1, 5, 2], [70000, -5, 0, 2], [3, 3, 3, -1]],
                      np.int32)


def band_thresholds(params: dict) -> dict:
    return {k: params[k] for k in ("pixel_thresh", "depth_thresh", "min_conf") if k in params}


BEHIND_DEPTH = 6.0
BEHIND_PIXELS = {"nan_inf": [(36, 18), (36, 23)], "inf_nan": [(30, 20)], "inf_inf": [(31, 15), (44, 27)]}  # (x, y) of A


@functools.lru_cache(maxsize=None)
def make_behind_scene(W: int = 72, H: int = 40, seed: int = 5) -> Scene:
    """Three views, no tracks. A (view 0) and B (view 1) have the identity rotation and dyadic centres (0.5, -0.25, 0)
    and (0.5, -0.25, 6): B sits inside the sphere, past its front, looking at the plane. Every sphere pixel of A nearer
    than z = 6 lies behind B. A's principal point is the integer pixel (36, 20), so that pixel's point is on B's
    principal ray, exactly: it transfers to (0, 0, z < 0) and projects to B's principal point. The pixels of
    BEHIND_PIXELS carry the depth 6 exactly and transfer to z = 0 exactly (the products with the identity's zeros and
    the sums with dyadic centres are exact): on A's principal column x = 0 as well, so u = f 0 / 0 + u0 is NaN and v
    infinite; on its principal row the other way round; elsewhere both are infinite. C (view 2) looks at the sphere
    from the side with a third set of intrinsics and gives A and B an ordinary source."""
    rng = np.random.default_rng(seed)
    centres = np.array([[0.5, -0.25, 0.0], [0.5, -0.25, BEHIND_DEPTH], [2.25, 0.3, 0.5]])
    wRc = np.stack([np.eye(3), np.eye(3), look_at(centres[2], SPHERE_C)])
    intr = np.array([[FOCAL_PER_WIDTH * W, 36.0, 20.0], [70.0, 33.5, 21.5], [85.0, 38.2, 17.6]])
    clean = render_depth(wRc, centres, intr, H, W)
    depth = clean.astype(F32)
    for pixels in BEHIND_PIXELS.values():
        for x, y in pixels:
            depth[0, y, x] = F32(BEHIND_DEPTH)
    conf = rng.uniform(0.6, 1.0, (3, H, W)).astype(F32)
    images = rng.integers(0, 256, (3, H, W, 3)).astype(np.uint8)
    none = np.zeros(0, np.int32)
    return Scene(wRc, centres, intr, np.ones(3, np.uint8), np.zeros(1, np.int32), none, np.zeros((0, 3)),
                 np.zeros(0, np.uint8), np.zeros(0, np.uint8), H, W, depth, conf, images, clean, -1)


PERCENTILE_LENGTHS = (1, 2, 3, 101, 102, 257, 1025)  # (n - 1) 0.01 = 1 at 101; past one and past four workgroups


def percentile_edge_lists(seed: int = 21):
    """{(kind, n): float64 list} for the depth-list lengths above: all negative; mixed sign with -0.0 beside +0.0; all
    equal; values that differ only in the lowest byte (the last of the eight radix passes); values that differ only in
    sign and exponent (the first pass and the top half of the second)."""
    rng = np.random.default_rng(seed)
    out = {}
    for n in PERCENTILE_LENGTHS:
        out["negative", n] = -rng.uniform(4.0, 40.0, n)
        mixed = rng.normal(0.0, 3.0, n)
        mixed[0] = -0.0
        if n > 1:
            mixed[1] = 0.0
        out["mixed", n] = mixed
        out["equal", n] = np.full(n, -7.3)
        base = np.array([5.3]).view(np.int64)[0] & ~np.int64(255)
        out["low_byte", n] = (base + rng.integers(0, 256, n)).astype(np.int64).view(np.float64)
        out["sign_exponent", n] = rng.choice([-1.0, 1.0], n) * np.ldexp(1.37, rng.integers(-20, 21, n))
    return out


def valid_cameras(s: Scene):
    v = np.flatnonzero(s.cam_keep)
    return s.wRc[v], s.wtc[v], s.intr[v]


def band_margins(s: Scene):
    """The threshold band of the fusion checks: (dist margin in pixels, rel margin, confidence margin).

    The device and this restatement run the same IEEE operations in the same order, so they are expected to agree
    exactly; the band only allows for the one place where a last-bit difference is amplified: the float32 source
    coordinate. One float32 ulp of the largest coordinate (below 256 here: 2^-16 pixel) moves the sample by that much,
    and the sampled depth by at most ulp * G, where G is the scene's largest depth difference between neighbouring
    pixels (the corrupted maps included). That depth error moves rel by ulp * G / d_min, and the reprojected pixel by at
    most f * B / d_min^2 per unit of depth (B the longest baseline, the parallax of a depth change), to which one ulp of
    the float32 reprojected coordinate is added. Confidence is compared as stored, with no arithmetic: its margin is 0."""
    ulp = 2.0 ** -16
    d = np.where(np.isfinite(s.depth) & (s.depth > 0), s.depth, np.nan)
    G = max(np.nanmax(np.abs(np.diff(np.nan_to_num(s.depth, nan=0.0), axis=1))),
            np.nanmax(np.abs(np.diff(np.nan_to_num(s.depth, nan=0.0), axis=2))))
    d_min = float(np.nanmin(d))
    _, wtc, intr = valid_cameras(s)
    B = max(np.linalg.norm(a - b) for a in wtc for b in wtc)
    m_depth = ulp * float(G)
    return ulp + intr[:, 0].max() * B / d_min ** 2 * m_depth, m_depth / d_min + 2.0 ** -23, 0.0  # the largest f


def band(s: Scene, ref: FusedRef, pixel_thresh=1.0, depth_thresh=0.01, min_conf=0.8) -> np.ndarray:
    """(n, H, W) bool: pixels within the margins of a threshold for any source."""
    m_dist, m_rel, m_conf = band_margins(s)
    with np.errstate(invalid="ignore"):
        b = (np.abs(ref.dist - pixel_thresh) <= m_dist).any(1) | \
            (np.abs(ref.rel.astype(np.float64) - float(F32(depth_thresh))) <= m_rel).any(1)
    return b | (np.abs(s.conf.astype(np.float64) - float(F32(min_conf))) < m_conf)
