"""The dense-MVS geometry kernels (gtsfm_mvs_*) and gtsfm_amd.densify on the MI355X against the numpy restatement
(tests/mvs_ref.py), on the analytic scene whose conditions tests/test_mvs.py asserts on the CPU: six valid cameras on an
arc (image 3 dropped, so image index != pm_i), a plane with a sphere in front of it, maps of 72 x 40 and 136 x 24
(widths no multiple of 64, H W no multiple of the 256-lane workgroup, several workgroups per view), 5 % wrong depths,
a few 0 / NaN / negative ones, confidence around 0.8, one view with no confident pixel, a source looking aside.

The threshold band. Device and restatement run the same IEEE operations in the same order and are expected to agree
bit for bit; masks and fused depth are still compared only outside a band around the three thresholds, derived in
mvs_ref.band_margins: one float32 ulp of the largest source coordinate (2^-16 below 256) times the scene's largest
depth difference between neighbouring pixels G bounds the error of the sampled depth; divided by the smallest depth it
bounds rel; times the parallax f B / d_min^2, plus one ulp, it bounds dist. The CPU test asserts that at most 1 % of a
view's pixels lie in the band.
"""
import functools

import numpy as np
import pytest
import torch

from tests import mvs_ref as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(72, 40), (136, 24)]


def _t(a, dtype=None):
    if a is None:
        return None
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))).to(DEV)


def _cameras(s):
    return _t(s.wRc), _t(s.wtc), _t(s.intr), _t(s.cam_keep)


class _Csr:
    def __init__(self, s):
        self.offsets, self.image = _t(s.offsets), _t(s.img)


@functools.lru_cache(maxsize=None)
def _views_ref(shape, max_num_views=5, cam_keep=None):
    s = M.make_scene(*shape)
    keep = s.cam_keep if cam_keep is None else np.array(cam_keep, np.uint8)
    return M.select_views(s.offsets, s.img, s.point, s.track_keep, s.inlier, s.wRc, s.wtc, keep, max_num_views)


def _gpu_views(shape, max_num_views=5, cam_keep=None):
    from gtsfm_amd.densify.mvs_depth_fusion import select_views_arrays

    s = M.make_scene(*shape)
    cams = list(_cameras(s))
    if cam_keep is not None:
        cams[3] = _t(np.array(cam_keep, np.uint8))
    return select_views_arrays(tuple(cams), _Csr(s), _t(s.point), _t(s.track_keep), _t(s.inlier), max_num_views)


@functools.lru_cache(maxsize=None)
def _fused_ref(shape, n_src=4):
    s = M.make_scene(*shape)
    wRc, wtc, intr = M.valid_cameras(s)
    return M.fuse_depth(s.depth, s.conf, wRc, wtc, intr, _views_ref(shape, n_src + 1).src_views)


@functools.lru_cache(maxsize=None)
def _gpu_dense(shape, n_src=4):
    from gtsfm_amd.densify.mvs_depth_fusion import MvsViews, fuse_depth_arrays

    s = M.make_scene(*shape)
    v = _views_ref(shape, n_src + 1)  # the restatement's views: this test is about fusion alone
    views = MvsViews(_t(v.img_to_pm), _t(v.pm_to_img), None, None, _t(v.src_views), _t(v.depth_range), None)
    d = fuse_depth_arrays(_t(s.depth), _t(s.conf), _t(s.images), _cameras(s), views)
    torch.cuda.synchronize()
    return d


# ---------------------------------------------------------------- view selection
@pytest.mark.parametrize("max_num_views,cam_keep", [(5, None), (5, (1, 0, 0, 1, 0, 1, 0)), (2, None), (1, None),
                                                    (9, None)])
def test_select_views_against_the_restatement(max_num_views, cam_keep):
    """n_valid = 6 with V = 5; n_valid = 3 < max_num_views; one source; none; more views asked for than exist."""
    want = _views_ref(SHAPES[0], max_num_views, cam_keep)
    got = _gpu_views(SHAPES[0], max_num_views, cam_keep)
    assert got.img_to_pm.cpu().tolist() == want.img_to_pm.tolist()
    assert got.pm_to_img.cpu().tolist() == want.pm_to_img.tolist()
    fixed = got.scores_fixed.cpu().numpy()
    diff = np.abs(fixed - want.scores)
    print("largest score difference in units of 2^-40:", diff.max(), "terms per entry up to", want.terms.max())
    assert np.all(diff <= want.terms)
    np.testing.assert_array_equal(fixed, fixed.T)
    np.testing.assert_array_equal(got.scores.cpu().numpy(), fixed / M.SCORE_SCALE)
    assert got.src_views.shape == want.src_views.shape
    np.testing.assert_array_equal(got.src_views.cpu().numpy(), want.src_views)
    np.testing.assert_allclose(got.depth_range.cpu().numpy(), want.depth_range, rtol=1e-12, atol=0)
    assert got.stats.cpu().tolist() == want.stats.tolist()


def test_select_views_long_depth_list_and_camera_without_measurement():
    """5,000 measurements in one camera (several passes of the select over more values than a workgroup has lanes), one
    valid camera that no track sees: (NaN, NaN) and the flag."""
    from gtsfm_amd import device

    rng = np.random.default_rng(8)
    T = 5000
    offsets = np.arange(0, 2 * T + 1, 2, dtype=np.int32)
    img = np.tile(np.array([0, 2], np.int32), T)
    wRc = np.tile(np.eye(3), (3, 1, 1))
    wtc = np.array([[0.0, 0, 0], [5.0, 0, 0], [1.0, 0, 0]])
    point = np.concatenate([rng.uniform(-1, 1, (T, 2)), rng.uniform(4, 40, (T, 1))], 1)
    point[:7, 2] = point[7, 2]  # equal depths
    want = M.select_views(offsets, img, point, None, None, wRc, wtc, None, 3)
    r = device.mvs_select_views(_t(offsets), _t(img), _t(point), None, None, _t(wRc), _t(wtc), None, 3)
    rng_gpu = r.depth_range.cpu().numpy()
    np.testing.assert_allclose(rng_gpu[[0, 2]], want.depth_range[[0, 2]], rtol=1e-12, atol=0)
    assert want.depth_range[0, 0] == pytest.approx(np.percentile(point[:, 2], 1), rel=1e-14)
    assert np.isnan(rng_gpu[1]).all() and np.isnan(want.depth_range[1]).all()
    assert r.stats.cpu().tolist() == want.stats.tolist() == [3, 2, 1, T]
    assert r.src_views.cpu().tolist() == want.src_views.tolist() == [[2, 1], [0, 2], [0, 1]]


# ---------------------------------------------------------------- fusion
@pytest.mark.parametrize("shape,n_src", [(SHAPES[0], 4), (SHAPES[1], 4), (SHAPES[0], 1)])
def test_fuse_depth_against_the_restatement(shape, n_src):
    s = M.make_scene(*shape)
    want, got = _fused_ref(shape, n_src), _gpu_dense(shape, n_src)
    band = M.band(s, want)
    n = want.mask.shape[0]
    assert np.all(band.reshape(n, -1).mean(1) <= 0.01)
    mask, fused = got.mask.cpu().numpy(), got.fused.cpu().numpy()
    print("mask differences inside the band:", int((mask != want.mask)[band].sum()), "of", int(band.sum()))
    np.testing.assert_array_equal(mask[~band], want.mask[~band])
    joint = (mask & 4) != 0
    assert np.array_equal(joint, (mask & 3) == 3) and np.all(fused[~joint] == 0)
    both = joint & ~band
    rel = np.abs(fused[both].astype(np.float64) - want.fused[both]) / want.fused[both]
    print("largest relative fused-depth difference:", rel.max())
    assert rel.max() <= 1e-6
    # counts and error statistics agree with the masks the kernel returned
    counts, err = got.counts.cpu().numpy(), got.err.cpu().numpy()
    for bit, col in ((1, 0), (2, 1), (4, 2)):
        np.testing.assert_array_equal(counts[:, col], ((mask & bit) != 0).reshape(n, -1).sum(1))
    assert counts[s.dead_view, 2] == 0 and err[s.dead_view].tolist() == [0.0, 0.0, 0.0]
    # The expected statistics come from the kernel's own joint mask and the restatement's distances. Outside the band
    # "dist < threshold" is certain; a band pixel may fall either way, which bounds the count from both sides. Where
    # the count equals the restatement's over all joint pixels, every band pixel fell the restatement's way and sum,
    # minimum and maximum are checked exactly (the sum within half a unit of 2^-24 per term).
    exact = 0
    for r in range(n):
        near = want.dist[r] < 1.0                                   # (S, H, W), the restatement's distances
        sure, maybe = near & (joint[r] & ~band[r]), near & joint[r] | (joint[r] & band[r])
        assert sure.sum() <= counts[r, 3] <= maybe.sum()
        e = want.dist[r][near & joint[r]]
        if counts[r, 3] == len(e) and len(e):
            exact += 1
            assert err[r, 0] == pytest.approx(e.sum(), abs=len(e) * 2.0 ** -25 + 1e-12)
            assert err[r, 1] == e.min() and err[r, 2] == e.max()
        if counts[r, 3]:
            assert 0.0 <= err[r, 1] <= err[r, 0] / counts[r, 3] <= err[r, 2] < 1.0
    assert exact >= n - 2  # every view but the one without a joint pixel, and at most one more


@pytest.mark.parametrize("shape", SHAPES)
def test_points_colours_and_order(shape):
    s = M.make_scene(*shape)
    got = _gpu_dense(shape)
    wRc, wtc, intr = M.valid_cameras(s)
    v = _views_ref(shape)
    pts, cols, off = M.gather_points(got.fused.cpu().numpy(), got.mask.cpu().numpy(), wRc, wtc, intr, s.images,
                                     v.pm_to_img)
    assert len(pts) > 4000 and got.points.shape == pts.shape
    np.testing.assert_array_equal(got.view_offset.cpu().numpy(), off)
    assert off[s.dead_view] == off[s.dead_view + 1]
    np.testing.assert_allclose(got.points.cpu().numpy(), pts, rtol=0, atol=1e-9)  # also the canonical order
    np.testing.assert_array_equal(got.colors.cpu().numpy(), cols)


# ---------------------------------------------------------------- voxels
def test_voxel_stats_and_downsample():
    from gtsfm_amd import device
    from gtsfm_amd.densify import mvs_utils

    got = _gpu_dense(SHAPES[0])
    pts, cols = got.points.cpu().numpy(), got.colors.cpu().numpy()
    stats = device.mvs_voxel_stats(got.points)
    want = M.voxel_stats(pts)
    st = stats.cpu().numpy()
    np.testing.assert_allclose(st[0:3], want[0:3], rtol=1e-12)
    # 1e-12 relative, elementwise on the diagonal; the off-diagonal entries are sums that cancel and may be arbitrarily
    # small against their terms, so they are held to 1e-12 of the geometric mean of their two diagonal entries (the
    # bound of an entry by Cauchy-Schwarz), not of themselves
    S_got, S_want = st[3:12].reshape(3, 3), want[3:12].reshape(3, 3)
    np.testing.assert_allclose(np.diag(S_got), np.diag(S_want), rtol=1e-12, atol=0)
    scale = np.sqrt(np.outer(np.diag(S_want), np.diag(S_want)))
    assert np.all(np.abs(S_got - S_want) <= 1e-12 * scale)
    np.testing.assert_array_equal(S_got, S_got.T)
    np.testing.assert_array_equal(st[12:18], want[12:18])
    voxel, _ = mvs_utils.estimate_minimum_voxel_size_arrays(got.points)
    assert voxel == pytest.approx(M.voxel_size(want, len(pts)), rel=1e-9) and voxel > 0
    voxel *= 20  # several points per voxel
    r = device.mvs_voxel_downsample(got.points, got.colors, stats, voxel)
    w_p, w_c, w_k, w_n = M.voxel_downsample(pts, cols, st[12:15], voxel)
    m = int(r.n_voxels.item())
    assert m == len(w_k) < len(pts) / 2 and w_n.max() > 3
    np.testing.assert_array_equal(r.keys[:m].cpu().numpy(), w_k)
    np.testing.assert_array_equal(r.count[:m].cpu().numpy(), w_n)
    np.testing.assert_allclose(r.points[:m].cpu().numpy(), w_p, rtol=0, atol=1e-12)
    np.testing.assert_array_equal(r.colors[:m].cpu().numpy(), w_c)
    assert not r.points[m:].any() and not r.count[m:].any()
    p2, c2 = mvs_utils.downsample_point_cloud_arrays(got.points, got.colors, voxel)
    assert p2.shape == (m, 3) and torch.equal(p2, r.points[:m]) and torch.equal(c2, r.colors[:m])
    p3, c3 = mvs_utils.downsample_point_cloud(pts, cols, voxel)
    np.testing.assert_array_equal(p3, p2.cpu().numpy())
    assert mvs_utils.downsample_point_cloud_arrays(got.points, got.colors, 0.0)[0] is got.points
    with pytest.raises(ValueError, match="voxels"):  # more voxels along an axis than the keys hold
        mvs_utils.downsample_point_cloud_arrays(got.points, got.colors, (st[15:18] - st[12:15]).max() / 2 ** 21)
    # on a stream that is not the current one: the sort between the two kernels runs there too
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    r_side = device.mvs_voxel_downsample(got.points, got.colors, stats, voxel, stream=side)
    side.synchronize()
    assert torch.equal(r_side.points, r.points) and torch.equal(r_side.keys, r.keys)
    assert mvs_utils.estimate_minimum_voxel_size(pts[:1]) == 0
    one = device.mvs_voxel_stats(got.points[:1].contiguous()).cpu().numpy()
    assert not one[3:12].any() and np.array_equal(one[0:3], pts[0])


# ---------------------------------------------------------------- determinism
def test_two_launches_byte_identical():
    from gtsfm_amd import device

    a, b = _gpu_views(SHAPES[1]), _gpu_views(SHAPES[1])
    for x, y in zip(a, b):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    d1 = _gpu_dense(SHAPES[1])
    _gpu_dense.cache_clear()
    d2 = _gpu_dense(SHAPES[1])
    for name, x, y in zip(d1._fields, d1, d2):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), name
    s1, s2 = device.mvs_voxel_stats(d1.points), device.mvs_voxel_stats(d1.points)
    assert s1.cpu().numpy().tobytes() == s2.cpu().numpy().tobytes()
    v1 = device.mvs_voxel_downsample(d1.points, d1.colors, s1, 0.05)
    v2 = device.mvs_voxel_downsample(d1.points, d1.colors, s1, 0.05)
    for f in ("points", "colors", "keys", "count", "n_voxels"):
        assert getattr(v1, f).cpu().numpy().tobytes() == getattr(v2, f).cpu().numpy().tobytes(), f


# ---------------------------------------------------------------- arguments
def test_argument_checks():
    from gtsfm_amd import device, native

    L = native.lib()
    OK, ARG, CAP = native.GTSFM_OK, native.GTSFM_ERR_ARG, native.GTSFM_ERR_CAPACITY
    s = M.make_scene(*SHAPES[0])
    st = native.stream_handle()
    off, img, point, wRc, wtc = _t(s.offsets), _t(s.img), _t(s.point), _t(s.wRc), _t(s.wtc)
    T, n_meas, n_img = len(s.offsets) - 1, len(s.img), len(s.wtc)
    need = L.gtsfm_mvs_select_views_workspace_bytes(T, n_meas, n_img)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    i2p, p2i = torch.full((n_img,), 7, dtype=torch.int32, device=DEV), torch.empty(n_img, dtype=torch.int32, device=DEV)
    scores = torch.empty((n_img, n_img), dtype=torch.int64, device=DEV)
    src = torch.empty((n_img, 4), dtype=torch.int32, device=DEV)
    rng = torch.empty((n_img, 2), dtype=torch.float64, device=DEV)
    stats = torch.full((4,), -1, dtype=torch.int64, device=DEV)

    def select(off_p=off.data_ptr(), n_tracks=T, nbytes=need, views=5, stats_p=stats.data_ptr()):
        return L.gtsfm_mvs_select_views(off_p, img.data_ptr(), n_tracks, n_meas, point.data_ptr(), None, None,
                                        wRc.data_ptr(), wtc.data_ptr(), None, n_img, views, ws.data_ptr(), nbytes,
                                        i2p.data_ptr(), p2i.data_ptr(), scores.data_ptr(), src.data_ptr(),
                                        rng.data_ptr(), stats_p, st)

    assert select() == OK  # NULL optionals: every track, measurement and camera
    torch.cuda.synchronize()
    assert stats.cpu().tolist()[:2] == [n_img, 4] and i2p.cpu().tolist() == list(range(n_img))
    assert select(off_p=None) == ARG and select(stats_p=None) == ARG and select(n_tracks=-1) == ARG
    assert select(views=0) == ARG and select(nbytes=need - 1) == CAP
    assert select(n_tracks=0) == OK
    torch.cuda.synchronize()
    assert stats.cpu().tolist() == [0, 0, 0, 0] and not scores.any() and not i2p.any()

    n, H, W = s.depth.shape
    depth, conf = _t(s.depth), _t(s.conf)
    cams = [_t(a) for a in M.valid_cameras(s)]
    srcv = _t(_views_ref(SHAPES[0]).src_views)
    need = L.gtsfm_mvs_fuse_depth_workspace_bytes(n, H, W)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    fused = torch.empty((n, H, W), dtype=torch.float32, device=DEV)
    mask = torch.empty((n, H, W), dtype=torch.uint8, device=DEV)
    counts = torch.full((n, 4), -1, dtype=torch.int64, device=DEV)
    err = torch.full((n, 3), -1.0, dtype=torch.float64, device=DEV)

    def fuse(depth_p=depth.data_ptr(), n_views=n, height=H, nbytes=need, pix=1.0):
        return L.gtsfm_mvs_fuse_depth(depth_p, conf.data_ptr(), n_views, height, W, cams[0].data_ptr(),
                                      cams[1].data_ptr(), cams[2].data_ptr(), srcv.data_ptr(), 4, pix, 0.01, 0.8, 1,
                                      ws.data_ptr(), nbytes, fused.data_ptr(), mask.data_ptr(), counts.data_ptr(),
                                      err.data_ptr(), st)

    assert fuse() == OK
    assert fuse(depth_p=None) == ARG and fuse(n_views=-1) == ARG and fuse(pix=float("nan")) == ARG
    assert fuse(pix=2048.0) == ARG and fuse(nbytes=need - 1) == CAP
    assert fuse(n_views=0) == OK and fuse(height=0) == OK
    torch.cuda.synchronize()
    assert not counts.any() and not err.any()
    with pytest.raises(native.NativeError):
        device.mvs_fuse_depth(depth, conf, *cams, srcv, workspace_bytes=need - 1)
    # no source at all: nothing is consistent, nothing is joint with min_consistent_views = 1
    r = device.mvs_fuse_depth(depth, conf, *cams, srcv[:, :0].contiguous())
    assert not r.counts[:, [0, 2, 3]].any() and not r.fused.any()
    pts, cols, voff = device.mvs_gather_points(r.fused, r.mask, *cams, _t(s.images), None, 0)
    assert pts.shape == (0, 3) and voff.cpu().tolist() == [0] * (n + 1)
    images = _t(s.images)
    need = L.gtsfm_mvs_gather_points_workspace_bytes(n, H, W)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    voff = torch.full((n + 1,), -1, dtype=torch.int64, device=DEV)

    def gather(n_views=n, nbytes=need, capacity=0, voff_p=voff.data_ptr()):
        return L.gtsfm_mvs_gather_points(r.fused.data_ptr(), r.mask.data_ptr(), n_views, H, W, cams[0].data_ptr(),
                                         cams[1].data_ptr(), cams[2].data_ptr(), images.data_ptr(), None,
                                         images.shape[0], images.shape[1], images.shape[2], capacity, ws.data_ptr(),
                                         nbytes, None, None, voff_p, st)

    assert gather() == OK and gather(nbytes=need - 1) == CAP
    assert gather(n_views=-1) == ARG and gather(capacity=-1) == ARG and gather(voff_p=None) == ARG
    assert gather(capacity=5) == ARG  # a capacity without buffers
    assert gather(n_views=0) == OK
    with pytest.raises(native.NativeError):
        device.mvs_gather_points(r.fused, r.mask, *cams, _t(s.images[:, :8]), None, 0)  # an image smaller than the maps
    empty = torch.empty((0, 3), dtype=torch.float64, device=DEV)
    assert not device.mvs_voxel_stats(empty).any()
    v = device.mvs_voxel_downsample(empty, torch.empty((0, 3), dtype=torch.uint8, device=DEV),
                                    device.mvs_voxel_stats(empty), 1.0)
    assert int(v.n_voxels.item()) == 0
    assert L.gtsfm_mvs_voxel_stats(None, -1, None, 0, stats.data_ptr(), st) == ARG
    vstats = torch.empty(18, dtype=torch.float64, device=DEV)
    need = L.gtsfm_mvs_voxel_stats_workspace_bytes(300)
    assert L.gtsfm_mvs_voxel_stats(point.data_ptr(), 300, ws.data_ptr(), need, vstats.data_ptr(), st) == OK
    assert L.gtsfm_mvs_voxel_stats(point.data_ptr(), 300, ws.data_ptr(), need - 1, vstats.data_ptr(), st) == CAP
    assert L.gtsfm_mvs_voxel_stats(point.data_ptr(), 300, ws.data_ptr(), need, None, st) == ARG
    assert L.gtsfm_mvs_voxel_keys(point.data_ptr(), -1, vstats.data_ptr(), 1.0, scores.data_ptr(), st) == ARG
    assert L.gtsfm_mvs_voxel_keys(None, 3, vstats.data_ptr(), 1.0, scores.data_ptr(), st) == ARG
    assert L.gtsfm_mvs_voxel_downsample(point.data_ptr(), mask.data_ptr(), scores.data_ptr(), scores.data_ptr(), -1,
                                        ws.data_ptr(), need, point.data_ptr(), mask.data_ptr(), scores.data_ptr(),
                                        src.data_ptr(), stats.data_ptr(), st) == ARG
    assert L.gtsfm_mvs_voxel_keys(point.data_ptr(), 3, stats.data_ptr(), 0.0, scores.data_ptr(), st) == ARG
    assert L.gtsfm_mvs_voxel_downsample(point.data_ptr(), mask.data_ptr(), scores.data_ptr(), scores.data_ptr(), 3,
                                        ws.data_ptr(), 8, point.data_ptr(), mask.data_ptr(), scores.data_ptr(),
                                        src.data_ptr(), stats.data_ptr(), st) == CAP


# ---------------------------------------------------------------- the stage
def _analytic_estimator(images, proj_inputs, depth_range):
    wRc, wtc, intr, src_views = proj_inputs
    n, H, W, _ = images.shape
    d = M.render_depth(wRc.cpu().numpy(), wtc.cpu().numpy(), intr.cpu().numpy(), H, W)
    return _t(d, np.float32), torch.full((n, H, W), 0.95, dtype=torch.float32, device=DEV)


def test_stage_with_the_analytic_estimator_and_run():
    """MVSDepthFusion over the scene's tracks with the analytic renderer as the depth estimator: images of 75 x 44 are
    cropped to 72 x 40 from the top-left corner, every point lies on the plane or the sphere within the 1 % depth
    threshold, and run() downsamples the cloud."""
    from gtsfm_amd.bundle.bundle_adjustment import BaData
    from gtsfm_amd.common import geometry as g
    from gtsfm_amd.common.image import Image
    from gtsfm_amd.common.sfm_track import SfmTrack
    from gtsfm_amd.densify.mvs_depth_fusion import MVSDepthFusion

    s = M.make_scene(*SHAPES[0])
    rng = np.random.default_rng(1)
    big = rng.integers(0, 256, (len(s.wtc), 44, 75, 3)).astype(np.uint8)
    mvs = MVSDepthFusion(_analytic_estimator)
    dense, views = mvs.densify_views(_t(big), _cameras(s), _Csr(s), _t(s.point), _t(s.track_keep), _t(s.inlier))
    assert dense.fused.shape == (6, 40, 72) and views.pm_to_img.cpu().tolist() == [0, 1, 2, 4, 5, 6]
    pts = dense.points.cpu().numpy()
    assert len(pts) > 0.5 * 6 * 40 * 72
    surface = np.minimum(np.abs(pts[:, 2] - M.PLANE_Z), np.abs(np.linalg.norm(pts - M.SPHERE_C, axis=1) - M.SPHERE_R))
    print("largest distance from the surface:", surface.max())
    assert surface.max() < 0.01 * 12.0  # 1 % of the largest depth in view
    first = np.flatnonzero((dense.mask[0].cpu().numpy() & 4).reshape(-1))[0]
    np.testing.assert_array_equal(dense.colors[0].cpu().numpy(), big[0, first // 72, first % 72])
    cams = {int(i): g.PinholeCameraCal3Bundler(g.Pose3(g.Rot3(s.wRc[i]), s.wtc[i]),
                                               g.Cal3Bundler(s.intr[i, 0], 0, 0, s.intr[i, 1], s.intr[i, 2]))
            for i in np.flatnonzero(s.cam_keep)}
    tracks = []
    for t in np.flatnonzero(s.track_keep):
        track = SfmTrack(s.point[t])
        for m in range(s.offsets[t], s.offsets[t + 1]):
            if s.inlier[m] and s.cam_keep[s.img[m]]:
                track.addMeasurement(int(s.img[m]), np.zeros(2))
        tracks.append(track)
    images = {i: Image(big[i]) for i in range(len(big))}
    p, c, metrics = mvs.densify(images, BaData(cams, tracks))
    np.testing.assert_array_equal(p, pts)
    assert len(metrics["joint_mask_valid_ratios"]) == 6 and metrics["reprojection_errors"]["count"] > len(pts)
    sp, sc, m2 = mvs.run(images, BaData(cams, tracks))
    assert 0 < len(sp) <= len(pts) and sc.shape == sp.shape and sc.dtype == np.uint8
    assert m2["point cloud size before downsampling"] == len(pts) and m2["voxel size for downsampling"] > 0
