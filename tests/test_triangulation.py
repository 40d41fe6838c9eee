"""tests/triangulation_ref.py pinned on the reference's known answers, and the CPU-side pieces of the triangulation.

The scene of the reference's tests/data_association/test_point3d_initializer.py is rebuilt: eight cameras on a circle
of radius 40 looking at the origin, f = 50, principal point 0 (gtsam.examples.SFMdata.createPoses is not installed, so
its poses are restated and checked to project the origin to (0, 0)); its Skydio two-camera case (:258-311); the three
num_ransac_hypotheses values it pins; and its door-dataset case on the committed fixture.
"""
import numpy as np
import pytest

import triangulation_ref as ref

DELTA = 1e-6  # the near-tie margin of tests/test_triangulation_gpu.py


def _circle_track(idx=range(8), shift=None):
    cams = ref.circle_cameras()
    idx = np.array(list(idx), np.int32)
    uv, z = ref.project(cams, idx, np.zeros((len(idx), 3)))
    if shift is not None:
        uv = uv + np.asarray(shift)
    return cams, np.array([0, len(idx)], np.int32), idx, uv


def _run(cams, off, img, uv, mode, thresh=5.0, n_hyp=100, **kw):
    return ref.triangulate_tracks(off, img, uv, cams, mode, thresh, n_hyp=n_hyp, **kw)


def test_circle_cameras_look_at_the_origin():
    cams = ref.circle_cameras()
    uv, z = ref.project(cams, np.arange(8), np.zeros((8, 3)))
    assert np.allclose(uv, 0.0, atol=1e-12) and (z > 0).all()
    assert np.allclose(np.linalg.norm(cams.wtc[:, :2], axis=1), 40.0)
    for R in cams.wRc:
        assert np.allclose(R @ R.T, np.eye(3)) and np.isclose(np.linalg.det(R), 1.0)


@pytest.mark.parametrize("mode", [ref.NO_RANSAC, ref.UNIFORM, ref.TOPK])
def test_circle_scene_known_answers(mode):
    cams, off, img, uv = _circle_track()
    r = _run(cams, off, img, uv, mode)
    assert r.exit_code[0] == ref.SUCCESS and np.allclose(r.point[0], 0.0) and r.inlier.all()
    r = _run(*_circle_track(range(2)), mode)
    assert r.exit_code[0] == ref.SUCCESS and np.allclose(r.point[0], 0.0)
    r = _run(*_circle_track(range(1)), mode)
    assert r.exit_code[0] == ref.INLIERS_UNDER and np.isnan(r.avg_err[0])
    shift = np.zeros((8, 2))
    shift[5] = (20.0, -10.0)
    r = _run(*_circle_track(shift=shift), mode)
    if mode == ref.NO_RANSAC:
        assert r.exit_code[0] == ref.EXCEEDS and not np.isnan(r.avg_err[0])
    else:
        assert r.exit_code[0] == ref.SUCCESS and np.allclose(r.point[0], 0.0)
        assert r.inlier.tolist() == [1, 1, 1, 1, 1, 0, 1, 1]
    flipped = cams._replace(wRc=cams.wRc @ np.diag([1.0, -1.0, -1.0]))  # yaw of pi: Rot3.RzRyRx(pi, 0, 0)
    r = _run(flipped, off, img, uv, mode)
    assert r.exit_code[0] != ref.SUCCESS
    if mode == ref.NO_RANSAC:
        assert r.exit_code[0] == ref.CHEIRALITY
    # a second, displaced measurement in camera 0
    img9 = np.concatenate([img, [0]]).astype(np.int32)
    uv9 = np.concatenate([uv, uv[:1] + np.array([[2.0, -3.0]])])
    r = _run(cams, np.array([0, 9], np.int32), img9, uv9, mode)
    assert r.exit_code[0] == ref.SUCCESS and np.allclose(r.point[0], 0.0, atol=1, rtol=1e-1)


def _skydio():
    wR1 = np.array([[-0.736357028, -0.589757459, 0.331608908], [0.565525823, -0.805544778, -0.176856308],
                    [0.371428151, 0.0573040157, 0.926691631]])
    wR2 = np.array([[-0.802732442, -0.594660358, 0.0447178336], [0.59626145, -0.80157983, 0.0440688035],
                    [0.009638943, 0.0620389785, 0.998027182]])
    wt1 = np.array([-0.649658109, 0.656963354, -0.382548681])
    wt2 = np.array([-1.95517763, 1.44100216, -0.442089696])
    return ref.Cameras(np.stack([np.eye(3), wR1, wR2]), np.stack([np.zeros(3), wt1, wt2]),
                       np.tile(np.array([583.1175, 507.0, 380.0]), (3, 1)), np.array([False, True, True]))


def test_unestimated_camera():
    cams = _skydio()
    r = _run(cams, np.array([0, 2], np.int32), np.array([0, 1], np.int32),
             np.array([[229.0, 500.0], [69.0, 532.0]]), ref.NO_RANSAC)
    assert r.exit_code[0] == ref.POSES_UNDER and np.isnan(r.avg_err[0])
    # length 3 with camera 0 unestimated: the point comes from cameras 1 and 2, camera 0's error is NaN: exit 4
    X = np.array([-1.0, 1.0, 3.0])
    uv12, z = ref.project(cams, np.array([1, 2]), np.tile(X, (2, 1)))
    assert (z > 0).all()
    r = _run(cams, np.array([0, 3], np.int32), np.array([0, 1, 2], np.int32),
             np.concatenate([[[229.0, 500.0]], uv12]), ref.NO_RANSAC)
    assert r.exit_code[0] == ref.EXCEEDS and np.allclose(r.point[0], X) and r.avg_err[0] < 1e-6


def test_num_ransac_hypotheses():
    from gtsfm_amd.frontend.triangulation_options import (TriangulationExitCode, TriangulationOptions,
                                                          TriangulationSamplingMode)

    mode = TriangulationSamplingMode.RANSAC_SAMPLE_UNIFORM
    assert TriangulationOptions(reproj_error_threshold=5, mode=mode).num_ransac_hypotheses() == 2749
    assert TriangulationOptions(reproj_error_threshold=5, mode=mode,
                                min_num_hypotheses=10000).num_ransac_hypotheses() == 10000
    assert TriangulationOptions(reproj_error_threshold=5, mode=mode, min_inlier_ratio=1e-4,
                                max_num_hypotheses=1000).num_ransac_hypotheses() == 1000
    with pytest.raises(AssertionError):
        TriangulationOptions(reproj_error_threshold=-1, mode=mode).num_ransac_hypotheses()
    assert [c.value for c in TriangulationExitCode] == [0, 1, 2, 3, 4, 5]
    assert TriangulationExitCode.EXCEEDS_REPROJ_THRESH.value == ref.EXCEEDS


def test_door_fixture_and_its_two_failures():
    off, img, uv, cams = ref.load_door()
    assert len(off) - 1 == 8824 and len(img) == 46493 and uv.dtype == np.float32
    lens = np.diff(off)
    assert lens.min() == 2 and lens.max() == 12
    r = _run(cams, off, img, uv, ref.NO_RANSAC, thresh=1e5)
    assert np.flatnonzero(r.exit_code != ref.SUCCESS).tolist() == [3668, 7439]
    assert (r.exit_code[[3668, 7439]] == ref.CHEIRALITY).all()
    # the reference's expected_failures (test_point3d_initializer.py:233-248)
    assert img[off[3668]: off[3669]].tolist() == [1, 2, 4] and img[off[7439]: off[7440]].tolist() == [6, 7, 9]
    assert np.allclose(uv[off[3668]], [1252.22729492, 1487.29431152])
    assert abs(np.nanmedian(r.avg_err) - 0.22) < 0.01


def test_door_near_ties_under_the_cap():
    """The restatement alone flags fewer than 1 % of the door's tracks at DELTA under the shipped options."""
    off, img, uv, cams = ref.load_door()
    r = _run(cams, off, img, uv, ref.UNIFORM, thresh=3.0, n_hyp=100)
    assert (np.diff(off) * (np.diff(off) - 1) // 2 <= 100).all()  # every track enumerates all its pairs
    share = r.margins.near_tie(DELTA).mean()
    print(f"near-ties at {DELTA}: {share:.5f}")
    assert share < 0.01


def test_selection_is_the_m_smallest_keys():
    off, img, uv, cams, _ = ref.make_synth()
    t = int(np.flatnonzero(np.diff(off) == 40)[0])
    im = img[off[t]: off[t + 1]]
    for mode in (ref.UNIFORM, ref.TOPK):
        js = ref.select_pairs(mode, 11, t, im, cams, 100)
        keys = ref.pair_keys(mode, 11, t, im, cams)
        assert len(js) == 100 and len(keys) == 780 and (np.diff(js) > 0).all()
        rest = np.setdiff1d(np.arange(780), js)
        assert keys[js].max() <= keys[rest].min()
    assert len(ref.select_pairs(ref.UNIFORM, 0, 0, im[:14], cams, 100)) == 91


def test_sfm_track_stand_in():
    from gtsfm_amd.common.sfm_track import SfmTrack

    tr = SfmTrack(np.array([1.0, 2.0, 3.0]))
    tr.addMeasurement(4, np.array([5.0, 6.0]))
    assert tr.numberMeasurements() == 1 and tr.point3().tolist() == [1.0, 2.0, 3.0]
    i, uv = tr.measurement(0)
    assert i == 4 and np.asarray(uv).tolist() == [5.0, 6.0]


def test_workspace_query_and_argument_errors_without_gpu():
    from gtsfm_amd import native

    lib = native.lib()
    q = lib.gtsfm_triangulate_workspace_bytes
    assert q(0, 10, 100) == 0 and q(10, 0, 100) == 0 and q(-1, 10, 100) == 0 and q(10, 10, -1) == 0
    assert q(1 << 31, 10, 100) == 0
    small, big = q(10, 40, 100), q(8824, 46493, 100)
    assert 0 < small < big
    assert q(1 << 20, 1 << 24, 2749) <= (1 << 20) * 8 + (64 << 20) + 8192  # the hypothesis buffer is capped
    assert q(10, 40, 100) >= 8 * 11 + 20 * 100  # one track's worst case always fits
    f = lib.gtsfm_triangulate_tracks
    nul = [None] * 3
    # the checks below fail before anything touches a device: negative sizes, unknown / unbuilt modes, bad threshold
    base = dict(n_tracks=1, n_meas=2, n_img=1, mode=0, thr=1.0, n_hyp=0)

    def call(**kw):
        a = dict(base, **kw)
        return f(*nul, 0, None, a["n_tracks"], None, a["n_meas"], None, None, None, None, a["n_img"], a["mode"],
                 a["thr"], 0.0, a["n_hyp"], 0, None, 0, None, None, None, None, None, None, None, 0, None)

    assert call(n_tracks=-1) == native.GTSFM_ERR_ARG
    assert call(n_meas=-1) == native.GTSFM_ERR_ARG
    assert call(mode=native.GTSFM_TRI_RANSAC_SAMPLE_BIASED_BASELINE) == native.GTSFM_ERR_ARG
    assert call(mode=7) == native.GTSFM_ERR_ARG
    assert call(thr=0.0) == native.GTSFM_ERR_ARG
    assert call(thr=float("nan")) == native.GTSFM_ERR_ARG
    assert call() == native.GTSFM_ERR_ARG  # d_stats is NULL
