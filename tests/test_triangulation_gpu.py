"""gtsfm_triangulate_tracks on the MI355X against tests/triangulation_ref.py (the reference route in numpy).

Decisions (exit codes, inlier bytes) must equal the restatement's on every track that is not a near-tie (a decision
margin below DELTA, see triangulation_ref.Margins); near-ties may be at most 1 % of the tracks. With DELTA = 1e-6 the
restatement flags 0 of the door fixture's 8,824 tracks under the shipped options (checked on the CPU in
tests/test_triangulation.py), so the cap binds.

Tolerance of point and avg_err: the restatement's own rounding floor, measured on the CPU by running it on the door
fixture (NO_RANSAC, threshold 1e5) twice, once with every track's measurements in reversed order (the same problem,
another summation order), and taking the maximum over non-near-tie tracks of |dX| / depth and of |d avg_err|:

    python -c "import sys; sys.path.insert(0, 'tests'); import triangulation_ref as R; print(R.rounding_floor())"
    -> (1.6e-14, 3.4e-13)

The GPU is held to FACTOR = 10 times that floor (one-sided Jacobi and LAPACK differ by more than summation order). The
floor is measured again by the module fixture, so the bound follows the numpy in use. The noise-free circle scene uses
np.allclose's defaults, the reference's own bar.
"""
import functools

import numpy as np
import pytest
import torch

import tracks_ref
import triangulation_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DELTA = 1e-6
NEAR_TIE_CAP = 0.01
FACTOR = 10.0


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _gpu(offsets, image, uv, cams, mode, thresh, min_angle=0.0, n_hyp=0, seed=0, cam_valid="cams", **kw):
    from gtsfm_amd import device

    valid = cams.valid.astype(np.uint8) if isinstance(cam_valid, str) else cam_valid
    res = device.triangulate_tracks(_t(np.asarray(offsets, np.int32)), _t(np.asarray(image, np.int32)), _t(uv),
                                    _t(cams.wRc), _t(cams.wtc), _t(cams.intr), _t(valid), mode, thresh, min_angle,
                                    n_hyp, seed, want_hypotheses=True, **kw)
    torch.cuda.synchronize()
    return res


def _np(res):
    return {k: getattr(res, k).cpu().numpy() for k in ("exit_code", "point", "avg_err", "inlier", "stats", "n_hyp",
                                                       "hyp_pair")}


@functools.lru_cache(maxsize=None)
def _door():
    return ref.load_door()


@functools.lru_cache(maxsize=None)
def _door_ref(mode, thresh, n_hyp):
    off, img, uv, cams = _door()
    return ref.triangulate_tracks(off, img, uv, cams, mode, thresh, n_hyp=n_hyp)


@functools.lru_cache(maxsize=None)
def _floor():
    return ref.rounding_floor()


def _check_decisions(got, want, offsets, label):
    """Exit codes and inlier bytes equal outside the near-ties, which stay under the cap."""
    tie = want.margins.near_tie(DELTA)
    share = tie.mean() if len(tie) else 0.0
    n_diff = int((got["exit_code"] != want.exit_code).sum())
    print(f"{label}: near-ties {int(tie.sum())} of {len(tie)}, exit codes differing anywhere {n_diff}, "
          f"stats {got['stats'].tolist()} (reference {want.stats.tolist()})")
    assert share <= NEAR_TIE_CAP, f"{label}: {share:.4f} of the tracks are near-ties"
    keep = ~tie
    np.testing.assert_array_equal(got["exit_code"][keep], want.exit_code[keep], err_msg=label)
    meas_keep = np.repeat(keep, np.diff(offsets))
    np.testing.assert_array_equal(got["inlier"][meas_keep], want.inlier[meas_keep], err_msg=label)
    return keep


def _check_values(got, want, keep, label):
    floor_x, floor_e = _floor()
    sel = keep & np.isfinite(want.point).all(axis=1)
    assert np.isfinite(got["point"][sel]).all(), label
    dx = np.linalg.norm(got["point"][sel] - want.point[sel], axis=1) / want.depth[sel]
    has_avg = keep & ~np.isnan(want.avg_err)
    de = np.abs(got["avg_err"][has_avg] - want.avg_err[has_avg])
    print(f"{label}: max |dX| / depth {dx.max() if len(dx) else 0:.3e} (bound {FACTOR * floor_x:.3e}), "
          f"max |d avg_err| {de.max() if len(de) else 0:.3e} (bound {FACTOR * floor_e:.3e})")
    assert np.isnan(got["avg_err"][keep & np.isnan(want.avg_err)]).all(), label
    assert (dx <= FACTOR * floor_x).all(), f"{label}: point off by {dx.max():.3e} of the depth"
    assert (de <= FACTOR * floor_e).all(), f"{label}: avg_err off by {de.max():.3e}"


# ---------------------------------------------------------------- reference-scene cases, through the plugin classes
def _circle_initializer(mode, cams=None, **opts):
    from gtsfm_amd.common import geometry as g
    from gtsfm_amd.data_association.point3d_initializer import Point3dInitializer, TriangulationOptions

    c = ref.circle_cameras() if cams is None else cams
    cam_dict = {i: g.PinholeCameraCal3Bundler(g.Pose3(g.Rot3(c.wRc[i]), c.wtc[i]), g.Cal3Bundler(50, 0, 0, 0, 0))
                for i in range(8)}
    return Point3dInitializer(cam_dict, TriangulationOptions(reproj_error_threshold=5, mode=mode, **opts))


def _circle_measurements():
    from gtsfm_amd.common.sfm_track import SfmMeasurement

    c = ref.circle_cameras()
    uv, _ = ref.project(c, np.arange(8), np.zeros((8, 3)))
    return [SfmMeasurement(i, uv[i]) for i in range(8)]


def _modes():
    from gtsfm_amd.data_association.point3d_initializer import TriangulationSamplingMode as M

    return M


@pytest.mark.parametrize("mode_name", ["NO_RANSAC", "RANSAC_SAMPLE_UNIFORM", "RANSAC_TOPK_BASELINES"])
def test_circle_scene_cases(mode_name):
    from gtsfm_amd.common.sfm_track import SfmMeasurement, SfmTrack2d
    from gtsfm_amd.data_association.point3d_initializer import TriangulationExitCode

    mode = _modes()[mode_name]
    opts = {} if mode_name == "NO_RANSAC" else {"min_num_hypotheses": 100}
    init = _circle_initializer(mode, **opts)
    meas = _circle_measurements()
    track, avg, code = init.triangulate(SfmTrack2d(meas))
    assert code == TriangulationExitCode.SUCCESS and np.allclose(track.point3(), 0.0)
    assert track.numberMeasurements() == 8 and avg is not None
    track, _, _ = init.triangulate(SfmTrack2d(meas[:2]))
    assert np.allclose(track.point3(), 0.0)
    track, avg, code = init.triangulate(SfmTrack2d(meas[:1]))
    assert track is None and avg is None and code == TriangulationExitCode.INLIERS_UNDERCONSTRAINED
    outlier = list(meas)
    outlier[5] = SfmMeasurement(5, meas[5].uv + np.array([20.0, -10.0]))
    track, _, code = init.triangulate(SfmTrack2d(outlier))
    if mode_name == "NO_RANSAC":
        assert track is None and code == TriangulationExitCode.EXCEEDS_REPROJ_THRESH
    else:
        assert np.allclose(track.point3(), 0.0) and track.numberMeasurements() == 7
        assert 5 not in [track.measurement(k)[0] for k in range(7)]
    c = ref.circle_cameras()
    flip = np.diag([1.0, -1.0, -1.0])  # Rot3.RzRyRx(pi, 0, 0): a rotation of pi about x
    flipped = c._replace(wRc=c.wRc @ flip)
    track, _, _ = _circle_initializer(mode, cams=flipped, **opts).triangulate(SfmTrack2d(meas))
    assert track is None
    dup = list(meas) + [SfmMeasurement(0, meas[0].uv + np.array([2.0, -3.0]))]
    track, _, _ = init.triangulate(SfmTrack2d(dup))
    assert np.allclose(track.point3(), 0.0, atol=1, rtol=1e-1)


def test_biased_baseline_is_not_built():
    from gtsfm_amd.common.sfm_track import SfmTrack2d

    init = _circle_initializer(_modes().RANSAC_SAMPLE_BIASED_BASELINE)
    with pytest.raises(NotImplementedError):
        init.triangulate(SfmTrack2d(_circle_measurements()))


def test_empty_camera_dict_raises():
    from gtsfm_amd.data_association.point3d_initializer import Point3dInitializer, TriangulationOptions

    with pytest.raises(ValueError):
        Point3dInitializer({}, TriangulationOptions(mode=_modes().NO_RANSAC))


# ---------------------------------------------------------------- door fixture
def test_door_no_ransac():
    off, img, uv, cams = _door()
    want = _door_ref(ref.NO_RANSAC, 1e5, 0)
    got = _np(_gpu(off, img, uv, cams, ref.NO_RANSAC, 1e5))
    assert np.flatnonzero(got["exit_code"] != 0).tolist() == [3668, 7439]
    keep = _check_decisions(got, want, off, "door NO_RANSAC")
    assert keep.all()
    np.testing.assert_array_equal(got["stats"], want.stats)
    _check_values(got, want, keep, "door NO_RANSAC")


def test_door_shipped_options():
    off, img, uv, cams = _door()
    want = _door_ref(ref.UNIFORM, 3.0, 100)
    got = _np(_gpu(off, img, uv, cams, ref.UNIFORM, 3.0, n_hyp=100))
    lens = np.diff(off)
    np.testing.assert_array_equal(got["n_hyp"], lens * (lens - 1) // 2)  # every track enumerates all its pairs
    np.testing.assert_array_equal(got["hyp_pair"][: want.stats[7]], want.hyp_pair)
    keep = _check_decisions(got, want, off, "door UNIFORM 100")
    _check_values(got, want, keep, "door UNIFORM 100")


def test_door_two_launches_byte_identical_and_chunks():
    """Two launches into separate buffers, and a launch with a workspace that forces many chunks: the same bytes."""
    from gtsfm_amd import native

    off, img, uv, cams = _door()
    a = _np(_gpu(off, img, uv, cams, ref.UNIFORM, 3.0, n_hyp=100))
    b = _np(_gpu(off, img, uv, cams, ref.UNIFORM, 3.0, n_hyp=100))
    full = native.lib().gtsfm_triangulate_workspace_bytes(len(off) - 1, len(img), 100)
    small = (len(off)) * 8 + 256 + 3 * 256 + 20 * 100 * 700  # room for 700 tracks' worst case: 13 chunks
    assert small < full
    c = _np(_gpu(off, img, uv, cams, ref.UNIFORM, 3.0, n_hyp=100, workspace_bytes=small))
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
        assert a[k].tobytes() == c[k].tobytes(), f"{k} depends on the chunking"


def test_reversed_track_order_is_byte_identical():
    """The same tracks in reversed order, each keyed by its original index: every track's outputs are the same bytes.
    n_hyp = 7 makes every track of five or more measurements choose its pairs by the hash."""
    off, img, uv, cams = _door()
    T = 2000
    off = off[: T + 1]
    lens = np.diff(off)
    a = _np(_gpu(off, img[: off[-1]], uv[: off[-1]], cams, ref.UNIFORM, 3.0, n_hyp=7, seed=5))
    order = np.arange(T)[::-1]
    idx = np.concatenate([np.arange(off[t], off[t + 1]) for t in order])
    off_r = np.concatenate([[0], np.cumsum(lens[order])]).astype(np.int32)
    b = _np(_gpu(off_r, img[idx], uv[idx], cams, ref.UNIFORM, 3.0, n_hyp=7, seed=5,
                 track_id=_t(order.astype(np.int32))))
    for k in ("exit_code", "point", "avg_err", "n_hyp"):
        assert a[k][order].tobytes() == b[k].tobytes(), k
    assert a["inlier"][idx].tobytes() == b["inlier"].tobytes()


# ---------------------------------------------------------------- synthetic scene: the selection path
@functools.lru_cache(maxsize=None)
def _synth():
    return ref.make_synth()


@pytest.mark.parametrize("n_hyp", [100, 7])
@pytest.mark.parametrize("mode", [ref.NO_RANSAC, ref.UNIFORM, ref.TOPK])
def test_synthetic_selection(mode, n_hyp):
    off, img, uv, cams, outl = _synth()
    lens = np.diff(off)
    assert {2, 3, 15, 16, 40} <= set(lens.tolist())
    want = ref.triangulate_tracks(off, img, uv, cams, mode, 3.0, n_hyp=n_hyp, seed=11)
    got = _np(_gpu(off, img, uv, cams, mode, 3.0, n_hyp=n_hyp, seed=11))
    label = f"synthetic mode {mode} n_hyp {n_hyp}"
    if mode != ref.NO_RANSAC:
        np.testing.assert_array_equal(got["n_hyp"], np.minimum(n_hyp, lens * (lens - 1) // 2), err_msg=label)
        # the evaluated pairs are those the restatement selects (the same integer hash / the same fp64 baseline key)
        np.testing.assert_array_equal(got["hyp_pair"][: want.stats[7]], want.hyp_pair, err_msg=label)
        assert got["stats"][7] == want.stats[7]
    keep = _check_decisions(got, want, off, label)
    _check_values(got, want, keep, label)
    # two views cannot see a displacement along the epipolar line, so a mask of two measurements (a two-measurement
    # track, or a hypothesis nothing else votes for) may hold an outlier; from three on, a >= 50 px outlier cannot sit
    # within 3 px of a point that two other measurements agree on
    n_in = np.add.reduceat(got["inlier"].astype(np.int64), off[:-1])
    ok_meas = np.repeat((got["exit_code"] == 0) & (n_in >= 3), lens)
    assert not (got["inlier"][ok_meas & outl]).any(), f"{label}: a gross outlier is inside a successful track's mask"


# ---------------------------------------------------------------- shape edges
@pytest.mark.parametrize("n_tracks", [0, 1, 63, 64, 65, 257])
def test_track_counts(n_tracks):
    off, img, uv, cams = _door()
    off = off[: n_tracks + 1]
    n_meas = int(off[-1])
    want = ref.triangulate_tracks(off, img[:n_meas], uv[:n_meas], cams, ref.UNIFORM, 3.0, n_hyp=100)
    got = _np(_gpu(off, img[:n_meas], uv[:n_meas], cams, ref.UNIFORM, 3.0, n_hyp=100))
    np.testing.assert_array_equal(got["stats"], want.stats)
    np.testing.assert_array_equal(got["exit_code"], want.exit_code)
    np.testing.assert_array_equal(got["inlier"], want.inlier)


def test_device_track_count():
    """n_tracks read on the device (the stats of the tracks call): tracks past it are not touched."""
    off, img, uv, cams = _door()
    n_dev = torch.tensor([100, 0, 0, 0, 0], dtype=torch.int64, device=DEV)
    n_meas = int(off[300])
    got = _np(_gpu(off[:301], img[:n_meas], uv[:n_meas], cams, ref.UNIFORM, 3.0, n_hyp=100, n_tracks_dev=n_dev))
    want = ref.triangulate_tracks(off[:101], img, uv, cams, ref.UNIFORM, 3.0, n_hyp=100)
    np.testing.assert_array_equal(got["exit_code"][:100], want.exit_code)
    np.testing.assert_array_equal(got["stats"], want.stats)
    assert np.isnan(got["point"][100:]).all() and not got["inlier"][off[100]:].any()


def test_invalid_cameras_null_valid_and_inf_threshold():
    off, img, uv, cams = _door()
    off, n_meas = off[:65], int(off[64])
    img, uv = img[:n_meas], uv[:n_meas]
    # a track whose cameras are all invalid; one camera unestimated elsewhere
    none_valid = cams._replace(valid=np.zeros(len(cams.valid), bool))
    for mode in (ref.NO_RANSAC, ref.UNIFORM):
        got = _np(_gpu(off, img, uv, none_valid, mode, 3.0, n_hyp=100))
        code = ref.POSES_UNDER if mode == ref.NO_RANSAC else ref.INLIERS_UNDER
        assert (got["exit_code"] == code).all() and np.isnan(got["avg_err"]).all()
    one_out = cams._replace(valid=np.arange(len(cams.valid)) != 2)
    for mode in (ref.NO_RANSAC, ref.UNIFORM):
        want = ref.triangulate_tracks(off, img, uv, one_out, mode, 3.0, n_hyp=100)
        got = _np(_gpu(off, img, uv, one_out, mode, 3.0, n_hyp=100))
        np.testing.assert_array_equal(got["exit_code"], want.exit_code)
        np.testing.assert_array_equal(got["inlier"], want.inlier)
    # cam_valid = NULL is "all valid"
    a = _np(_gpu(off, img, uv, cams, ref.UNIFORM, 3.0, n_hyp=100))
    b = _np(_gpu(off, img, uv, cams, ref.UNIFORM, 3.0, n_hyp=100, cam_valid=None))
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    # an infinite threshold: everything in front of its camera is an inlier
    want = ref.triangulate_tracks(off, img, uv, cams, ref.UNIFORM, np.inf, n_hyp=100)
    got = _np(_gpu(off, img, uv, cams, ref.UNIFORM, float("inf"), n_hyp=100))
    np.testing.assert_array_equal(got["exit_code"], want.exit_code)
    np.testing.assert_array_equal(got["inlier"], want.inlier)


def test_min_triangulation_angle():
    """Cameras 0 and 1 subtend 1 degree at the origin, cameras 0 and 2 subtend 90."""
    deg = np.deg2rad([0.0, 1.0, 90.0])
    cams = ref.lookat_cameras(np.stack([10 * np.cos(deg), 10 * np.sin(deg), np.zeros(3)], axis=1))
    uv, _ = ref.project(cams, np.arange(3), np.zeros((3, 3)))
    off = np.array([0, 2, 4], np.int32)
    img = np.array([0, 1, 0, 2], np.int32)
    m_uv = uv[img]
    for angle, want in ((0.0, [0, 0]), (5.0, [ref.LOW_ANGLE, 0]), (180.0, [ref.LOW_ANGLE, ref.LOW_ANGLE])):
        got = _np(_gpu(off, img, m_uv, cams, ref.NO_RANSAC, 3.0, min_angle=angle))
        assert got["exit_code"].tolist() == want, angle
        r = ref.triangulate_tracks(off, img, m_uv, cams, ref.NO_RANSAC, 3.0, min_angle=angle)
        assert r.exit_code.tolist() == want
        assert np.allclose(got["point"], 0.0) and not np.isnan(got["avg_err"]).any()


# ---------------------------------------------------------------- chain
def _scene_cameras(n_img):
    th = np.linspace(0, 2 * np.pi, n_img, endpoint=False)
    return ref.lookat_cameras(np.stack([10 * np.cos(th), 10 * np.sin(th), np.zeros(n_img)], axis=1))


def test_chain_from_tracks_on_device():
    """DsfTracksEstimator.run_arrays feeds triangulate_arrays with device tensors throughout; the result equals the
    route through host numpy."""
    from gtsfm_amd.common import geometry as g
    from gtsfm_amd.data_association.dsf_tracks_estimator import DsfTracksEstimator
    from gtsfm_amd.data_association.point3d_initializer import Point3dInitializer, TriangulationOptions

    scene = tracks_ref.make_scene(8, 300, 400, 0.5, seed=3)
    cams = _scene_cameras(8)
    cam_dict = {i: g.PinholeCameraCal3Bundler(g.Pose3(g.Rot3(cams.wRc[i]), cams.wtc[i]),
                                              g.Cal3Bundler(800, 0, 0, 500, 400)) for i in range(8)}
    init = Point3dInitializer(cam_dict, TriangulationOptions(reproj_error_threshold=3, max_num_hypotheses=100,
                                                             mode=_modes().RANSAC_SAMPLE_UNIFORM))
    est = DsfTracksEstimator()
    dev_tracks = est.run_arrays(_t(scene.pairs), _t(scene.offsets), _t(scene.v_corr), _t(scene.kp_count), scene.kmax,
                                kp_xy=_t(scene.kp_xy))
    assert dev_tracks.uv.is_cuda
    on_dev = init.triangulate_arrays(dev_tracks)
    assert all(a.is_cuda for a in on_dev)
    host_tracks = est.run_arrays(scene.pairs, scene.offsets, scene.v_corr, scene.kp_count, scene.kmax,
                                 kp_xy=scene.kp_xy)
    on_host = init.triangulate_arrays(host_tracks)
    assert len(on_host.exit_code) == len(host_tracks.offsets) - 1 > 0
    for a, b in zip(on_dev, on_host):
        assert a.cpu().numpy().tobytes() == b.tobytes()
    # the same without a host-known track count: capacity from the buffer, count from the tracks call's stats
    counted = init.triangulate_arrays(dev_tracks, n_tracks_dev=dev_tracks.stats)
    assert counted.exit_code.cpu().numpy().tobytes() == on_host.exit_code.tobytes()


def test_run_triangulation_equals_per_track():
    from gtsfm_amd.common import geometry as g
    from gtsfm_amd.common.sfm_track import SfmMeasurement, SfmTrack2d
    from gtsfm_amd.data_association.data_assoc import DataAssociation
    from gtsfm_amd.data_association.point3d_initializer import Point3dInitializer, TriangulationOptions

    off, img, uv, cams = _door()
    f, u0, v0 = cams.intr[0]
    cam_dict = {i: g.PinholeCameraCal3Bundler(g.Pose3(g.Rot3(cams.wRc[i]), cams.wtc[i]), g.Cal3Bundler(f, 0, 0, u0, v0))
                for i in range(len(cams.valid))}
    tracks = [SfmTrack2d([SfmMeasurement(int(img[k]), uv[k].astype(np.float64)) for k in range(off[t], off[t + 1])])
              for t in range(200)]
    opts = TriangulationOptions(reproj_error_threshold=3, max_num_hypotheses=100, mode=_modes().RANSAC_TOPK_BASELINES)
    da = DataAssociation(3, opts)
    sfm_tracks, errs, codes = da.run_triangulation(cam_dict, tracks)
    assert len(sfm_tracks) == len(errs) == len(codes) == 200
    init = Point3dInitializer(cam_dict, opts)
    for t in range(0, 200, 7):
        track, err, code = init.triangulate(tracks[t])
        assert code == codes[t] and err == errs[t]
        assert (track is None) == (sfm_tracks[t] is None)
        if track is not None:
            assert track.point3().tobytes() == sfm_tracks[t].point3().tobytes()
            assert track.numberMeasurements() == sfm_tracks[t].numberMeasurements()
    lens2 = [da.validate_track(s) for s in sfm_tracks]
    assert lens2 == [s is not None and s.numberMeasurements() >= 3 for s in sfm_tracks]
