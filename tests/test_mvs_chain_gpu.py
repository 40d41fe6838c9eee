"""MVSDepthFusion.densify_arrays on a real MultiViewOptimizer.run_arrays result, on the MI355X.

The scene is gtsfm_amd/synthetic.py's room: its cameras (render_scene's orbit, 10 views of 160 x 120, with the images it
renders) and its five room planes (floor and four walls; the room is convex and the cameras are inside it, so a
surface point is seen by every camera whose image it falls into). 500 points are sampled on the floor and the walls;
keypoints are their exact projections rounded to float32, relative poses are exact. run_arrays returns cameras and
landmarks in bundle adjustment's own gauge, so a similarity (Umeyama) is fitted from its camera centres to the scene's:
the depth estimator renders the planes analytically for the cameras it is given (proj_inputs), mapped through that
similarity, and divides the depths by its scale; the cloud is mapped the same way and must lie on the planes.

Surface tolerance: a fused depth is the mean of depths within 1 % (the depth threshold) of a depth rendered on the
surface, and the rendering error is the float32 rounding of the map, so a point lies within 1 % of the largest
rendered depth of the surface along its ray, measured here as the distance to the nearest plane.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_IMG, H, W = 10, 120, 160


def _t(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))).to(DEV)


def _planes():
    from gtsfm_amd import synthetic

    return synthetic._room_planes()


def render_room_depth(wRc, wtc, intr, height, width):
    """z-depth of the room's planes at the integer pixel coordinates (n, height, width); 0 where a ray leaves the room
    through the open top."""
    x, y = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    out = np.zeros((len(wtc), height, width))
    for i in range(len(wtc)):
        rays = np.stack([(x - intr[i][1]) / intr[i][0], (y - intr[i][2]) / intr[i][0], np.ones_like(x)], -1) @ wRc[i].T
        best = np.full((height, width), np.inf)
        for n_, d_, org, ua, va, ext_u, ext_v in _planes():
            denom = rays @ n_
            with np.errstate(divide="ignore", invalid="ignore"):
                t = -(n_ @ wtc[i] + d_) / denom
            p = wtc[i] + t[..., None] * rays
            u, v = (p - org) @ ua, (p - org) @ va
            ok = (t > 0.05) & (t < best) & (u >= 0) & (u <= ext_u) & (v >= 0) & (v <= ext_v)
            best = np.where(ok, t, best)
        out[i] = np.where(np.isfinite(best), best, 0.0)  # the rays have camera z = 1: t is the z-depth
    return out


def plane_distance(X):
    """Distance of points (N, 3) to the nearest room plane."""
    return np.min(np.stack([np.abs(X @ n_ + d_) for n_, d_, *_ in _planes()]), 0)


def umeyama(src, dst):
    """(s, R, t) with dst ~ s R src + t."""
    ms, md = src.mean(0), dst.mean(0)
    a, b = dst - md, src - ms
    U, S, Vt = np.linalg.svd(a.T @ b)
    sgn = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        sgn[2] = -1.0
    R = U @ np.diag(sgn) @ Vt
    s = np.sum(S * sgn) / np.sum(b * b)
    return s, R, md - s * R @ ms


@functools.lru_cache(maxsize=None)
def _scene():
    from gtsfm_amd import synthetic

    sc = synthetic.render_scene(n_images=N_IMG, height=H, width=W, device=DEV, tex_size=256)
    rng = np.random.default_rng(21)
    floor = np.stack([rng.uniform(-5, 5, 350), rng.uniform(-5, 5, 350), np.zeros(350)], 1)
    side = rng.integers(0, 4, 150)
    a, z = rng.uniform(-9, 9, 150), rng.uniform(0.2, 5.0, 150)
    walls = np.stack([np.where(side == 0, -10.0, np.where(side == 2, 10.0, a)),
                      np.where(side == 1, -10.0, np.where(side == 3, 10.0, a)), z], 1)
    pts = np.concatenate([floor, walls])
    assert plane_distance(pts).max() < 1e-12
    intr = sc.intrinsics
    pc = np.einsum("nji,npj->npi", sc.wRc, pts[None] - sc.wtc[:, None])  # (n_img, n_pts, 3)
    with np.errstate(divide="ignore", invalid="ignore"):
        uv = intr[:, None, 1:3] + intr[:, None, :1] * pc[..., :2] / pc[..., 2:3]
    sees = (pc[..., 2] > 0.5) & (uv[..., 0] >= 0) & (uv[..., 0] <= W - 1) & (uv[..., 1] >= 0) & (uv[..., 1] <= H - 1)
    coords, kp_of = [], np.full((N_IMG, len(pts)), -1)
    for i in range(N_IMG):
        p = np.flatnonzero(sees[i])
        coords.append(uv[i, p].astype(np.float32))
        kp_of[i, p] = np.arange(len(p))
    pairs, rows = [], []
    for i in range(N_IMG):
        for j in range(i + 1, N_IMG):
            both = np.flatnonzero(sees[i] & sees[j])
            if len(both) >= 15:
                pairs.append((i, j))
                rows.append(np.stack([kp_of[i, both], kp_of[j, both]], 1).astype(np.int32))
    pairs = np.array(pairs, np.int32)
    offsets = np.zeros(len(pairs) + 1, np.int32)
    np.cumsum([len(r) for r in rows], out=offsets[1:])
    i1, i2 = pairs[:, 0], pairs[:, 1]
    i2Ri1 = np.einsum("nji,njk->nik", sc.wRc[i2], sc.wRc[i1])
    i2Ui1 = np.einsum("nji,nj->ni", sc.wRc[i2], sc.wtc[i1] - sc.wtc[i2])
    i2Ui1 /= np.linalg.norm(i2Ui1, axis=1, keepdims=True)
    kp_count = np.array([len(c) for c in coords], np.int32)
    kmax = int(kp_count.max())
    kp_xy = np.zeros((N_IMG, kmax, 2), np.float32)
    for i, c in enumerate(coords):
        kp_xy[i, : len(c)] = c
    args = (pairs, i2Ri1, i2Ui1, np.ones(len(pairs), np.uint8), offsets, np.concatenate(rows), kp_count, kmax, kp_xy,
            intr, N_IMG)
    return sc, args


@functools.lru_cache(maxsize=None)
def _run_arrays():
    from gtsfm_amd.averaging.rotation.shonan import ShonanRotationAveraging
    from gtsfm_amd.averaging.translation.averaging_1dsfm import TranslationAveraging1DSFM
    from gtsfm_amd.bundle.bundle_adjustment import BundleAdjustmentOptimizer
    from gtsfm_amd.data_association.data_assoc import DataAssociation
    from gtsfm_amd.data_association.point3d_initializer import TriangulationOptions, TriangulationSamplingMode
    from gtsfm_amd.multi_view_optimizer import MultiViewOptimizer

    opt = MultiViewOptimizer(ShonanRotationAveraging(), TranslationAveraging1DSFM(),
                             DataAssociation(2, TriangulationOptions(TriangulationSamplingMode.NO_RANSAC, 3.0)),
                             BundleAdjustmentOptimizer())
    _, args = _scene()
    r = opt.run_arrays(*(a if isinstance(a, int) else _t(a) for a in args))
    torch.cuda.synchronize()
    return r


def _similarity(r):
    sc, _ = _scene()
    kept = np.flatnonzero(r.ba.cam_keep.cpu().numpy())
    return umeyama(r.ba.wtc.cpu().numpy().reshape(-1, 3)[kept], sc.wtc[kept])


def test_densify_arrays_on_a_run_arrays_result():
    from gtsfm_amd.densify.mvs_depth_fusion import MVSDepthFusion

    sc, _ = _scene()
    r = _run_arrays()
    assert r.ba is not None and int(r.ba.cam_keep.sum()) >= 8
    s, R, t = _similarity(r)
    kept = np.flatnonzero(r.ba.cam_keep.cpu().numpy())
    fit = s * r.ba.wtc.cpu().numpy().reshape(-1, 3)[kept] @ R.T + t - sc.wtc[kept]
    print("similarity scale", s, "largest camera-centre residual", np.abs(fit).max())
    seen = {}

    def estimator(images, proj_inputs, depth_range):
        wRc, wtc, intr, src_views = (a.cpu().numpy() for a in proj_inputs)
        n, h, w, _ = images.shape
        d = render_room_depth(np.einsum("ij,njk->nik", R, wRc), s * wtc @ R.T + t, intr, h, w) / s
        seen.update(depth=d, depth_range=depth_range.cpu().numpy(), src=src_views)
        return _t(d, np.float32), torch.full((n, h, w), 0.95, dtype=torch.float32, device=DEV)

    mvs = MVSDepthFusion(estimator)
    dense, views = mvs.densify_arrays(sc.images, r)
    nv = len(kept)
    assert views.pm_to_img.cpu().tolist() == kept.tolist() and dense.fused.shape == (nv, H, W)
    assert seen["src"].shape == (nv, min(5, nv) - 1) and not np.isnan(seen["depth_range"]).any()
    # the depth ranges from the landmarks bracket most of what the renderer sees, in the same gauge
    assert np.all(seen["depth_range"][:, 0] > 0) and np.all(seen["depth_range"][:, 0] < seen["depth_range"][:, 1])
    pts = dense.points.cpu().numpy()
    assert len(pts) > 0.3 * nv * H * W and np.isfinite(pts).all()
    assert int(dense.view_offset[-1]) == len(pts) == int(dense.counts[:, 2].sum())
    surface = plane_distance(s * pts @ R.T + t)
    tol = 0.01 * s * seen["depth"].max()
    print("points", len(pts), "largest distance from the room's planes", surface.max(), "tolerance", tol)
    assert surface.max() <= tol
    first = np.flatnonzero((dense.mask[0].cpu().numpy() & 4).reshape(-1))[0]
    np.testing.assert_array_equal(dense.colors[0].cpu().numpy(),
                                  sc.images[int(kept[0]), first // W, first % W].cpu().numpy())


def test_densify_arrays_without_a_bundle_adjustment_result():
    """A chain that stopped early (ba is None) is refused by name, not by an attribute error deep inside."""
    from gtsfm_amd.densify.mvs_depth_fusion import MVSDepthFusion

    sc, _ = _scene()
    r = _run_arrays()._replace(ba=None)
    with pytest.raises(ValueError, match="bundle adjustment"):
        MVSDepthFusion(lambda *a: None).densify_arrays(sc.images, r)
