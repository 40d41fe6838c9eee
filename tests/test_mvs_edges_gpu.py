"""The dense-MVS kernels (gtsfm_mvs_*) on the MI355X where tests/test_mvs_gpu.py does not take them: past the first pass
of every scan and grid stride, with cameras that differ from one another, with the fusion parameters off their defaults
and ragged source rows, with a source the points lie behind, and with depth lists at the edges of the percentile.

A. Sizes just past a loop boundary (256 lanes per workgroup, 1,024 lanes per scan pass, 1,024 statistics workgroups):
   maps of 516 x 520 = 1,049 workgroups per view, 1,030 views, 300,000 points, 1,100 images.
B. Fusion on mvs_ref.make_scene(**mvs_ref.UNEQUAL), whose conditions (the 1 % band cap per parameter set, joint and
   non-joint pixels in every live view) tests/test_mvs.py asserts on the CPU; the comparison is the one of
   tests/test_mvs_gpu.py::test_fuse_depth_against_the_restatement with the thresholds in use.
C. mvs_select_views on one camera per depth list of mvs_ref.percentile_edge_lists.
"""
import functools
import math

import numpy as np
import pytest
import torch

from tests import mvs_ref as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -53


def _t(a, dtype=None):
    if a is None:
        return None
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))).to(DEV)


def _random_cameras(rng, n):
    """n cameras with unrelated rotations, centres and intrinsics."""
    centres = rng.normal(0.0, 1.0, (n, 3))
    look = rng.normal(0.0, 1.0, (n, 3)) + np.array([0.0, 0.0, 3.0])
    wRc = np.stack([M.look_at(c, c + d) for c, d in zip(centres, look)])
    return wRc, centres


# ---------------------------------------------------------------- A1, A2: gather
def _gather_both(fused, mask, wRc, wtc, intr, images, view_image, capacity=None):
    from gtsfm_amd import device

    want = M.gather_points(fused, mask, wRc, wtc, intr, images, view_image)
    cap = len(want[0]) if capacity is None else capacity
    got = device.mvs_gather_points(_t(fused), _t(mask), _t(wRc), _t(wtc), _t(intr), _t(images),
                                   _t(view_image, np.int32), cap)
    torch.cuda.synchronize()
    return want, got


def test_gather_more_than_1024_workgroups_per_view():
    """Two views of 516 x 520: 268,320 pixels in 1,049 workgroups, the last one with 32 pixels, so ga_scan_view_kernel
    runs a second pass and carries `base` into it. All eight mask bytes, ~30 % joint, runs of whole workgroups without
    a joint pixel on both sides of workgroup 1,024, 5,497 consecutive joint pixels; distinct (f, cx, cy) per view,
    images of 530 x 524 taken in swapped order. Then the same with half the capacity."""
    W, H, hw = 516, 520, 516 * 520
    assert -(-hw // 256) == 1049 and hw % 256 == 32
    rng = np.random.default_rng(31)
    mask = rng.choice(8, size=(2, hw), p=[0.7 / 4] * 4 + [0.3 / 4] * 4).astype(np.uint8)
    mask[0, 256 * 37:256 * 40] &= 3
    mask[0, 256 * 1023:256 * 1025] &= 3
    mask[1, 256 * 1030:256 * 1033] &= 3
    mask[1, 100_003:105_500] |= 4
    mask[:, 0] = mask[:, -1] = 7
    assert len(np.unique(mask)) == 8 and 0.28 < ((mask & 4) != 0).mean() < 0.33
    mask = mask.reshape(2, H, W)
    fused = rng.uniform(0.5, 30.0, (2, H, W)).astype(np.float32)
    wRc, wtc = _random_cameras(rng, 2)
    intr = np.array([[600.0, 250.3, 262.1], [480.5, 259.7, 255.4]])
    images = rng.integers(0, 256, (2, 524, 530, 3)).astype(np.uint8)
    view_image = np.array([1, 0])
    (pts, cols, off), (g_pts, g_cols, g_off) = _gather_both(fused, mask, wRc, wtc, intr, images, view_image)
    assert off[1] > 70_000 and off[2] - off[1] > 70_000
    np.testing.assert_array_equal(g_off.cpu().numpy(), off)
    np.testing.assert_array_equal(g_cols.cpu().numpy(), cols)
    np.testing.assert_allclose(g_pts.cpu().numpy(), pts, rtol=0, atol=1e-9)
    cap = int(off[2]) // 2
    assert 0 < cap < off[2]
    _, (h_pts, h_cols, h_off) = _gather_both(fused, mask, wRc, wtc, intr, images, view_image, cap)
    assert h_pts.shape == (cap, 3) and h_cols.shape == (cap, 3)
    assert torch.equal(h_off, g_off) and torch.equal(h_pts, g_pts[:cap]) and torch.equal(h_cols, g_cols[:cap])


def test_gather_more_than_1024_views():
    """1,030 views of 8 x 8, one workgroup each: ga_scan_kernel runs a second pass over the views. view_image is a
    permutation into 1,031 images with two entries of -1 and one of 5,000: those views are black. Views on both sides of
    view 1,024 have no joint pixel."""
    n = 1030
    rng = np.random.default_rng(32)
    mask = rng.choice(8, size=(n, 8, 8), p=[0.7 / 4] * 4 + [0.3 / 4] * 4).astype(np.uint8)
    mask[[3, 1023, 1024, 1027]] &= 3
    mask[[0, 1025, n - 1], 7, 7] = 7
    fused = rng.uniform(0.5, 30.0, (n, 8, 8)).astype(np.float32)
    wRc, wtc = _random_cameras(rng, n)
    intr = np.stack([rng.uniform(8.0, 12.0, n), rng.uniform(2.0, 5.0, n), rng.uniform(2.0, 5.0, n)], 1)
    images = rng.integers(1, 256, (n + 1, 8, 8, 3)).astype(np.uint8)  # no black pixel of its own
    view_image = rng.permutation(n + 1)[:n]
    view_image[[7, 1026]] = -1
    view_image[500] = 5000
    assert (view_image != np.arange(n)).mean() > 0.99
    (pts, cols, off), (g_pts, g_cols, g_off) = _gather_both(fused, mask, wRc, wtc, intr, images, view_image)
    assert off[1023] == off[1024] == off[1025] < off[1026] and off[n] > off[n - 1] and off[3] == off[4]
    np.testing.assert_array_equal(g_off.cpu().numpy(), off)
    np.testing.assert_array_equal(g_cols.cpu().numpy(), cols)
    np.testing.assert_allclose(g_pts.cpu().numpy(), pts, rtol=0, atol=1e-9)
    c = g_cols.cpu().numpy()
    for v in (7, 500, 1026):
        assert off[v + 1] > off[v] and not c[off[v]:off[v + 1]].any()
    assert c.any(1).sum() == len(c) - sum(off[v + 1] - off[v] for v in (7, 500, 1026))


# ---------------------------------------------------------------- A3: voxels
VOXEL = 0.0625
CLOUD_LO = np.array([2.5, -2.5, 6.5])


@functools.lru_cache(maxsize=None)
def _cloud():
    """300,000 points around (3, -2, 7): the corner CLOUD_LO itself (the minimum bound, dyadic, so that the grid's
    origin CLOUD_LO - VOXEL / 2 and every face origin + k VOXEL are exact), a uniform box of extent 1, five clusters of
    600 points each inside one voxel, and 2,000 points with one to three coordinates exactly on a voxel face."""
    rng = np.random.default_rng(41)
    n, n_face = 300_000, 2000
    box = CLOUD_LO + rng.uniform(0.0, 1.0, (n - 1 - 5 * 600 - n_face, 3))
    clusters = [c + rng.normal(0.0, 2e-4, (600, 3)) for c in CLOUD_LO + rng.uniform(0.2, 0.8, (5, 3))]
    k = rng.integers(1, 16, (n_face, 3))
    on_face = rng.random((n_face, 3)) < 0.5
    on_face[:, 0] |= ~on_face.any(1)
    face = (CLOUD_LO - VOXEL / 2) + k * VOXEL
    face = np.where(on_face, face, face + rng.uniform(0.0, 1.0, (n_face, 3)) * VOXEL)
    pts = np.concatenate([CLOUD_LO[None], box] + clusters + [face])
    cols = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    return pts, cols, k, on_face


def test_voxels_above_262144_points():
    """300,000 points: vs_mean_kernel and vs_scatter_kernel stride over their grid of 1,024 workgroups (lanes below
    37,856 take two points), vx_scan_kernel scans 1,172 workgroup counts in two passes.

    The fp64 sums are checked against exact values (math.fsum; long double with pairwise sums for the scatter, whose
    own error of some 64 units of 2^-64 is added to the bound) within L u sum |x_i|, u = 2^-53, for a sum whose longest
    chain of dependent additions is L (each addition errs by at most u times its result, and every partial result is
    at most sum |x_i| up to second order). Reading the kernels at n = 300,000 with a grid of 1,024 x 256 lanes:
      vs_mean_kernel / vs_scatter_kernel: ceil(n / 262,144) = 2 strided terms per lane, 6 butterfly steps, 4 waves added
      in order; the finish kernel: 1,024 partial sums over 256 lanes = 4 terms per lane, 6 butterfly steps, 4 waves.
      L = 2 + 6 + 4 + 4 + 6 + 4 = 26.
    The mean adds the division by n: (L + 1) u sum |x_i| / n. A scatter term rounds two subtractions and a product
    before it is added, and the sum is divided by n - 1: (L + 4) u sum |c_j c_k| / (n - 1); the kernel centres on its
    own mean, which moves the exact sum by n d_j d_k with d the mean's error. Off the diagonal sum |c_j c_k| is replaced
    by its Cauchy-Schwarz bound sqrt(sum c_j^2 sum c_k^2), as in tests/test_mvs_gpu.py. A voxel's mean adds its m points
    one after the other and divides: m u sum |x_i| / m."""
    from gtsfm_amd import device

    pts, cols, k, on_face = _cloud()
    n = len(pts)
    assert n == 300_000 > 262_144 and -(-n // 256) == 1172 > 1024
    assert np.array_equal(pts.min(0), CLOUD_LO) and (pts[:, 1] < 0).all() and (pts[:, 0] > 0).all()
    d_pts, d_cols = _t(pts), _t(cols)
    stats = device.mvs_voxel_stats(d_pts)
    st = stats.cpu().numpy()
    L = -(-n // (1024 * 256)) + 6 + 4 + 1024 // 256 + 6 + 4
    assert L == 26
    exact_mean = np.array([math.fsum(pts[:, j]) for j in range(3)]) / n  # the sum is exact, the division rounds once
    abs_sum = np.array([math.fsum(np.abs(pts[:, j])) for j in range(3)])
    mean_bound = (L + 2) * U * abs_sum / n  # + 1 for the kernel's division, + 1 for the division just above
    print("mean: difference", np.abs(st[0:3] - exact_mean), "bound", mean_bound, "L", L)
    assert np.all(np.abs(st[0:3] - exact_mean) <= mean_bound)
    assert np.finfo(np.longdouble).nmant >= 63
    c = pts.astype(np.longdouble) - exact_mean.astype(np.longdouble)
    S_want = np.array([[np.sum(c[:, j] * c[:, k2]) for k2 in range(3)] for j in range(3)]) / (n - 1)
    T = np.array([float(np.sum(c[:, j] * c[:, j])) for j in range(3)])
    cs = np.sqrt(np.outer(T, T))  # on the diagonal sum c_j^2 itself
    scatter_bound = ((L + 4) * U + 64 * 2.0 ** -64) * cs / (n - 1) + n * np.outer(mean_bound, mean_bound) / (n - 1)
    S_got = st[3:12].reshape(3, 3)
    diff = np.abs(S_got - S_want).astype(np.float64)
    print("scatter: difference", diff.tolist(), "bound", scatter_bound.tolist())
    assert np.all(diff <= scatter_bound)
    np.testing.assert_array_equal(S_got, S_got.T)
    np.testing.assert_array_equal(st[12:15], pts.min(0))
    np.testing.assert_array_equal(st[15:18], pts.max(0))

    keys = M.voxel_keys(pts, st[12:15], VOXEL)
    idx = np.stack([keys >> 42, (keys >> 21) & (2 ** 21 - 1), keys & (2 ** 21 - 1)], 1)
    assert np.array_equal(idx[-len(k):][on_face], k[on_face]) and on_face.all(1).sum() > 100  # a face belongs above
    r = device.mvs_voxel_downsample(d_pts, d_cols, stats, VOXEL)
    w_p, w_c, w_k, w_n = M.voxel_downsample(pts, cols, st[12:15], VOXEL)
    m = int(r.n_voxels.item())
    assert m == len(w_k) and 4000 < m < 17 ** 3 + 1 and w_n.max() > 300
    np.testing.assert_array_equal(r.keys[:m].cpu().numpy(), w_k)
    np.testing.assert_array_equal(r.count[:m].cpu().numpy(), w_n)
    np.testing.assert_array_equal(r.colors[:m].cpu().numpy(), w_c)
    order = np.argsort(keys, kind="stable")
    ends = np.cumsum(w_n)
    v_mean = np.zeros((m, 3))
    v_bound = np.zeros((m, 3))
    for j, (lo, hi) in enumerate(zip(ends - w_n, ends)):
        p = pts[order[lo:hi]]
        for a in range(3):
            v_mean[j, a] = math.fsum(p[:, a]) / (hi - lo)
            v_bound[j, a] = (hi - lo + 1) * U * math.fsum(np.abs(p[:, a])) / (hi - lo)
    v_diff = np.abs(r.points[:m].cpu().numpy() - v_mean)
    print("voxel means: largest difference", v_diff.max(), "its bound", v_bound[np.unravel_index(v_diff.argmax(), v_diff.shape)],
          "smallest bound / difference", (v_bound / np.maximum(v_diff, 1e-300)).min())
    assert np.all(v_diff <= v_bound)
    np.testing.assert_array_equal(r.points[:m].cpu().numpy(), w_p)  # the restatement adds in the kernel's order
    assert not r.points[m:].any() and not r.count[m:].any() and not r.keys[m:].any()


# ---------------------------------------------------------------- A4: view selection
@functools.lru_cache(maxsize=None)
def _ring():
    """1,100 cameras on a circle of radius 10 looking inward, about one in 15 dropped, 4,000 tracks of 2 to 4 cameras
    at most 15 places apart (triangulation angles up to some 14 degrees) on points near the centre. Twelve kept cameras
    are left out of those tracks and get by hand: no measurement (two), one partner (four), two (four), three (two)."""
    rng = np.random.default_rng(51)
    n_img = 1100
    ang = 2.0 * np.pi * np.arange(n_img) / n_img
    wtc = np.stack([10.0 * np.cos(ang), 0.2 * np.sin(7.0 * ang), 10.0 * np.sin(ang)], 1)
    wRc = np.stack([M.look_at(c, rng.normal(0.0, 0.3, 3)) for c in wtc])
    cam_keep = np.ones(n_img, np.uint8)
    cam_keep[rng.choice(n_img, n_img // 15, replace=False)] = 0
    kept = np.flatnonzero(cam_keep)
    sparse = [int(c) for c in rng.choice(kept, 12, replace=False)]
    tracks = []
    while len(tracks) < 4000:
        c0 = int(rng.integers(n_img))
        cams = (c0 + np.sort(rng.choice(np.arange(-15, 16), int(rng.integers(2, 5)), replace=False))) % n_img
        cams = [int(c) for c in cams if c not in sparse]
        if cams:
            tracks.append(cams)
    for i, c in enumerate(sparse[2:]):
        partners = [[1], [1], [1], [1], [1, 2], [1, 2], [1, 2], [1, 2], [1, 2, 3], [1, 2, 3]][i]
        tracks.append([c] + [int((c + 3 * p) % n_img) for p in partners if (c + 3 * p) % n_img not in sparse])
    offsets = np.cumsum([0] + [len(t) for t in tracks]).astype(np.int32)
    img = np.concatenate(tracks).astype(np.int32)
    r, a = 3.0 * np.sqrt(rng.random(len(tracks))), rng.uniform(0, 2 * np.pi, len(tracks))
    point = np.stack([r * np.cos(a), rng.uniform(-0.5, 0.5, len(tracks)), r * np.sin(a)], 1)
    return offsets, img, point, wRc, wtc, cam_keep, sparse


def test_select_views_over_more_than_1024_images():
    """sv_map_kernel and sv_scan_kernel run a second pass over the images; sv_src_kernel's lanes stride 17 times over
    1,026 valid views, most of them tied at a score of zero. The sources are checked against mvs_ref.source_views of
    the device's own fixed-point matrix, so that a score that differs from the restatement's by a unit can neither hide
    nor fake a wrong pick; the matrix itself is held to the restatement within one unit per term."""
    from gtsfm_amd import device

    offsets, img, point, wRc, wtc, cam_keep, sparse = _ring()
    want = M.select_views(offsets, img, point, None, None, wRc, wtc, cam_keep, 5)
    nv = len(want.pm_to_img)
    assert len(wtc) == 1100 and 1024 < nv < 1100 - 60
    partners = (want.scores > 0).sum(1)
    few = np.sort(partners[want.img_to_pm[sparse]])  # a hand-made partner may itself be a dropped camera
    assert (want.scores == 0).mean() > 0.95 and few[:2].tolist() == [0, 0] and few[2] == 1 and few[-1] <= 3
    assert (partners < 4).sum() >= 10 and want.stats[2] == 2
    r = device.mvs_select_views(_t(offsets), _t(img), _t(point), None, None, _t(wRc), _t(wtc), _t(cam_keep), 5)
    torch.cuda.synchronize()
    assert r.img_to_pm.cpu().tolist() == want.img_to_pm.tolist()
    assert r.pm_to_img.cpu().tolist()[:nv] == want.pm_to_img.tolist() and r.pm_to_img.cpu().tolist()[nv:] == [-1] * (1100 - nv)
    scores = r.scores.cpu().numpy()
    fixed = scores[:nv, :nv]
    assert not scores[nv:].any() and not scores[:, nv:].any()
    diff = np.abs(fixed - want.scores)
    print("largest score difference in units of 2^-40:", diff.max(), "terms per entry up to", want.terms.max())
    assert np.all(diff <= want.terms)
    np.testing.assert_array_equal(fixed, fixed.T)
    src = r.src_views.cpu().numpy()
    assert src.shape == (1100, 4)
    np.testing.assert_array_equal(src[:nv], M.source_views(fixed, 5))
    assert np.all(src[nv:] == -1)
    np.testing.assert_allclose(r.depth_range.cpu().numpy()[:nv], want.depth_range, rtol=1e-12, atol=0)
    assert np.isnan(want.depth_range).all(1).sum() == want.stats[2]
    assert r.stats.cpu().tolist() == want.stats.tolist()


# ---------------------------------------------------------------- B: fusion
def _device_kw(params):
    names = dict(pixel_thresh="pixel_thresh", depth_thresh="depth_thresh", min_conf="min_confidence",
                 min_views="min_consistent_views")
    return {names[k]: v for k, v in params.items()}


@functools.lru_cache(maxsize=None)
def _unequal():
    s = M.make_scene(72, 40, **M.UNEQUAL)
    v = M.select_views(s.offsets, s.img, s.point, s.track_keep, s.inlier, s.wRc, s.wtc, s.cam_keep)
    return s, v.src_views, v.pm_to_img


def _fuse_and_compare(s, src, view_image, params, tag):
    """The comparison of tests/test_mvs_gpu.py::test_fuse_depth_against_the_restatement for the thresholds of params,
    then the gather on the kernel's own result. Returns (restatement, device masks)."""
    from gtsfm_amd import device

    wRc, wtc, intr = M.valid_cameras(s)
    want = M.fuse_depth(s.depth, s.conf, wRc, wtc, intr, src, **params)
    cams = (_t(wRc), _t(wtc), _t(intr))
    got = device.mvs_fuse_depth(_t(s.depth), _t(s.conf), *cams, _t(src), **_device_kw(params))
    torch.cuda.synchronize()
    pixel_thresh = params.get("pixel_thresh", 1.0)
    band = M.band(s, want, **M.band_thresholds(params))
    n = want.mask.shape[0]
    print(tag, "band pixels per view:", band.reshape(n, -1).sum(1).tolist(), "joint per view:", want.counts[:, 2].tolist())
    assert np.all(band.reshape(n, -1).mean(1) <= 0.01)
    mask, fused = got.mask.cpu().numpy(), got.fused.cpu().numpy()
    print(tag, "mask differences inside the band:", int((mask != want.mask)[band].sum()), "of", int(band.sum()))
    np.testing.assert_array_equal(mask[~band], want.mask[~band])
    joint = (mask & 4) != 0
    assert np.array_equal(joint, (mask & 3) == 3) and np.all(fused[~joint] == 0)
    both = joint & ~band
    rel = np.abs(fused[both].astype(np.float64) - want.fused[both]) / want.fused[both]
    print(tag, "largest relative fused-depth difference:", rel.max())
    assert rel.max() <= 1e-6
    counts, err = got.counts.cpu().numpy(), got.err.cpu().numpy()
    for bit, col in ((1, 0), (2, 1), (4, 2)):
        np.testing.assert_array_equal(counts[:, col], ((mask & bit) != 0).reshape(n, -1).sum(1))
    if s.dead_view >= 0:
        assert counts[s.dead_view, 2] == 0 and err[s.dead_view].tolist() == [0.0, 0.0, 0.0]
    exact = 0
    for r in range(n):
        near = want.dist[r] < pixel_thresh  # NaN, so False, where the entry of src is no view
        sure, maybe = near & (joint[r] & ~band[r]), near & joint[r] | (joint[r] & band[r])
        maybe = maybe & np.isfinite(want.dist[r])
        assert sure.sum() <= counts[r, 3] <= maybe.sum()
        e = want.dist[r][near & joint[r]]
        if counts[r, 3] == len(e) and len(e):
            exact += 1
            assert err[r, 0] == pytest.approx(e.sum(), abs=len(e) * 2.0 ** -25 + 1e-12)
            assert err[r, 1] == e.min() and err[r, 2] == e.max()
        if counts[r, 3]:
            assert 0.0 <= err[r, 1] <= err[r, 0] / counts[r, 3] <= err[r, 2] < pixel_thresh
        else:
            assert err[r].tolist() == [0.0, 0.0, 0.0]
    assert exact >= (want.counts[:, 3] > 0).sum() - 1  # every view with an error to count, and at most one fewer
    # gather on what the kernel returned: the camera of the view lifts, the image of the view colours
    pts, cols, off = M.gather_points(fused, mask, wRc, wtc, intr, s.images, view_image)
    g_pts, g_cols, g_off = device.mvs_gather_points(got.fused, got.mask, *cams, _t(s.images), _t(view_image, np.int32),
                                                    len(pts))
    np.testing.assert_array_equal(g_off.cpu().numpy(), off)
    assert np.isfinite(g_pts.cpu().numpy()).all() and np.isfinite(fused).all()
    np.testing.assert_allclose(g_pts.cpu().numpy(), pts, rtol=0, atol=1e-9)
    np.testing.assert_array_equal(g_cols.cpu().numpy(), cols)
    return want, mask


@pytest.mark.parametrize("name", list(M.FUSION_PARAMS))
def test_fuse_unequal_cameras(name):
    """B1 (the default thresholds) and B2: f from 69 to 91, principal points up to 5 and 3 pixels off the middle and
    different in every view, so that the lift, the projection into the source, the lift there and the projection back
    each need the right camera; two and three required views of four sources, every threshold tightened at once, and
    no required view, where a pixel without a usable depth must still not pass."""
    s, src, pm_to_img = _unequal()
    want, mask = _fuse_and_compare(s, src, pm_to_img, M.FUSION_PARAMS[name], name)
    unusable = ~(np.isfinite(s.depth) & (s.depth > 0))
    assert unusable.reshape(len(mask), -1).sum(1).min() >= 7 and not (mask[unusable] & 5).any()
    if name == "zero_views":
        assert np.all((mask[~unusable] & 1) == 1)


@pytest.mark.parametrize("min_views", [1, 2])
def test_fuse_ragged_source_rows(min_views):
    """B3: rows with gaps, without any source, with an entry equal to n_views and far outside, and with one source two
    and three times: the restatement skips and counts as the kernel's loop does."""
    s, _, pm_to_img = _unequal()
    want, mask = _fuse_and_compare(s, M.RAGGED_SRC, pm_to_img, dict(min_views=min_views), f"ragged min_views={min_views}")
    assert not (mask[1] & 5).any() and want.counts[0, 2] > 0


def test_fuse_source_the_points_lie_behind():
    """B4: view 1 of mvs_ref.make_behind_scene has a quarter of view 0's points behind it, one of them exactly on its
    principal ray, and five at z = 0 exactly, where the projection is NaN or infinite: mv_sample's border path."""
    s = M.make_behind_scene()
    src = np.array([[1, 2], [0, 2], [0, 1]], np.int32)
    want, mask = _fuse_and_compare(s, src, np.arange(3), {}, "behind")
    for pixels in M.BEHIND_PIXELS.values():
        for x, y in pixels:
            assert mask[0, y, x] == want.mask[0, y, x] and not mask[0, y, x] & 1
    assert mask[0, 20, 36] == want.mask[0, 20, 36]
    # with the source behind as the only one, nothing of view 0 that lies behind it is consistent
    from gtsfm_amd import device

    wRc, wtc, intr = M.valid_cameras(s)
    alone = np.array([[1], [0], [-1]], np.int32)
    got = device.mvs_fuse_depth(_t(s.depth), _t(s.conf), _t(wRc), _t(wtc), _t(intr), _t(alone))
    ref = M.fuse_depth(s.depth, s.conf, wRc, wtc, intr, alone)
    band = M.band(s, ref)
    np.testing.assert_array_equal(got.mask.cpu().numpy()[~band], ref.mask[~band])
    x, y = np.meshgrid(np.arange(72.0), np.arange(40.0))
    z = M._transfer(wRc[0], wtc[0], intr[0], wRc[1], wtc[1], x, y, s.depth[0].astype(np.float64))[2]
    assert (z <= 0).mean() > 0.2 and not (got.mask.cpu().numpy()[0][z <= 0] & 1).any()


# ---------------------------------------------------------------- C: percentiles
def test_percentile_edges():
    """One camera per list of mvs_ref.percentile_edge_lists, every measurement a track of its own at (-1, -1, z) seen by
    a camera at the origin with the identity rotation: its depth is 0 (-1) + 0 (-1) + z = z exactly, -0.0 included."""
    from gtsfm_amd import device

    lists = M.percentile_edge_lists()
    names = list(lists)
    img = np.concatenate([np.full(len(lists[k]), c, np.int32) for c, k in enumerate(names)])
    z = np.concatenate([lists[k] for k in names])
    point = np.stack([np.full(len(z), -1.0), np.full(len(z), -1.0), z], 1)
    offsets = np.arange(len(z) + 1, dtype=np.int32)
    wRc, wtc = np.tile(np.eye(3), (len(names), 1, 1)), np.zeros((len(names), 3))
    r = device.mvs_select_views(_t(offsets), _t(img), _t(point), None, None, _t(wRc), _t(wtc), None, 1)
    got = r.depth_range.cpu().numpy()
    assert r.stats.cpu().tolist() == [len(names), 0, 0, 0]
    for c, k in enumerate(names):
        want = [M.percentile(lists[k], 0.01), M.percentile(lists[k], 0.99)]
        np.testing.assert_allclose(got[c], want, rtol=1e-12, atol=0, err_msg=str(k))
