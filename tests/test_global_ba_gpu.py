"""gtsfm_global_ba on the MI355X against the PCG restatement (tests/global_ba_ref.py).

Scenes (global_ba_ref.ring_scene: cameras on a ring looking at a unit cube of points, f = 1000, 0.5 px noise, 5 % of the
measurements displaced by 30 px), the smallest shapes at which each path can go wrong:
  small   5 cameras x 40 points, track lengths 2-5: everything inside one wave;
  medium  12 cameras x 300 points, lengths 2-7 (more than 64 measurements per camera), robust on and off, plus an invalid
          camera, a valid camera no track sees, an invalid track, a measurement switched off and a landmark behind its
          cameras;
  dense   3 cameras x 400 points all seen by all: 400 measurements per camera, past the 256 lanes of a camera workgroup.
The seeds leave the restatement a decision margin above 1e-6 on every configuration (tests/test_global_ba.py checks
that on the CPU), so LM iterations, trials, the keep masks and the counters must equal the restatement's.

Tolerances: the largest GPU-to-restatement difference measured over these scenes and the door fixture, times 10 for the
different summation order ("Global bundle adjustment"); the ceiling is ba2.hip's bar against its oracle,
1e-4 degrees and 1e-6 relative. MEASURED holds the measured maxima, TOL the bars.
"""
import functools

import numpy as np
import pytest
import torch

import global_ba_ref as ref
import triangulation_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
THRESH = 3.0
#            rotation (deg), translation, points, error (all but the first relative)
MEASURED = dict(rot=7.7e-10, trans=1.3e-11, point=7.2e-11, err=5.2e-12)
TOL = {k: 10.0 * v for k, v in MEASURED.items()}
CEILING = dict(rot=1e-4, trans=1e-6, point=1e-6, err=1e-6)
assert all(TOL[k] <= CEILING[k] for k in TOL)
CONFIGS = (("small", 1, True), ("medium", 6, True), ("medium", 6, False), ("dense", 2, True))
SCENES = {"small": ref.scene_small, "medium": ref.scene_medium, "dense": ref.scene_dense}


def _t(a, dtype=None):
    if a is None:
        return None
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))
    return torch.from_numpy(a).to(DEV)


def _gpu(s, **kw):
    from gtsfm_amd import device

    r = device.global_ba(_t(s["offsets"], np.int32), _t(s["img"], np.int32), _t(s["uv"]), _t(s["point"]),
                         _t(s["track_valid"], np.uint8), _t(s["meas_valid"], np.uint8), _t(s["wRc"]), _t(s["wtc"]),
                         _t(s["intr"]), _t(s["cam_valid"], np.uint8), **kw)
    return {k: getattr(r, k).cpu().numpy() for k in ("wRc", "wtc", "point", "track_keep", "cam_keep", "stats")}


@functools.lru_cache(maxsize=None)
def _case(name, seed, robust):
    s = SCENES[name](seed)
    want = ref.global_ba_ref(*ref.call_args(s), robust=robust, reproj_error_thresh=THRESH)
    got = _gpu(s, robust=robust, reproj_error_thresh=THRESH)
    return s, want, got


def _counts_equal(gpu, want, label):
    """LM iterations, trials and PCG cap hits equal. The PCG total is not a decision with a margin: each solve ends
    when ||r|| crosses 1e-10 ||b||, the residual falls by a small factor per iteration, and a crossing that rounding
    moves costs one iteration more or less; it is held to 2 iterations per trial."""
    np.testing.assert_array_equal(gpu[[2, 3, 5]], want[[2, 3, 5]], err_msg=label)
    assert abs(gpu[4] - want[4]) <= 2 * want[3], f"{label}: PCG iterations {gpu[4]} vs {want[4]}"


def _compare(label, s, want, got):
    """Counts and masks equal (the LM and PCG counts only where the restatement's decisions have a margin); poses,
    points and errors within TOL. Prints every figure before asserting."""
    cams = np.nonzero(np.asarray(s["cam_valid"], bool) & np.isin(np.arange(len(want.wRc)), s["img"]))[0]
    rot, tr = ref.pose_diff(got["wRc"], got["wtc"], want.wRc, want.wtc, cams)
    nan = np.isnan(want.point)  # landmarks the triangulation left undefined are copied through as they are
    np.testing.assert_array_equal(np.isnan(got["point"]), nan, err_msg=label)
    dp = np.abs(got["point"] - want.point)[~nan].max() / np.abs(want.point[~nan]).max()
    de = max(abs(got["stats"][k] - want.stats[k]) / max(abs(want.stats[k]), 1e-300) for k in (0, 1))
    print(f"{label}: rot {rot:.3e} deg, trans {tr:.3e}, point {dp:.3e}, error {de:.3e}; stats gpu "
          f"{got['stats'].tolist()} ref {want.stats.tolist()}; ref margin {want.min_margin:.2e}")
    if want.min_margin > 1e-6:
        _counts_equal(got["stats"], want.stats, label)
    np.testing.assert_array_equal(got["stats"][6:], want.stats[6:], err_msg=label)
    np.testing.assert_array_equal(got["track_keep"], want.track_keep, err_msg=label)
    np.testing.assert_array_equal(got["cam_keep"], want.cam_keep, err_msg=label)
    assert rot <= TOL["rot"] and tr <= TOL["trans"] and dp <= TOL["point"] and de <= TOL["err"], label


@pytest.mark.parametrize("name,seed,robust", CONFIGS)
def test_matches_restatement(name, seed, robust):
    s, want, got = _case(name, seed, robust)
    assert want.min_margin > 1e-6  # the seeds are chosen for it (tests/test_global_ba.py)
    _compare(f"{name} robust={robust}", s, want, got)
    assert got["stats"][1] < got["stats"][0] and got["stats"][9] == 0


def test_non_entries_are_the_inputs_bit_for_bit():
    s, want, got = _case("medium", 6, True)
    e = s["edge"]
    for c in (e["invalid_cam"], e["unseen_cam"]):
        assert np.array_equal(got["wRc"][c], s["wRc"][c]) and np.array_equal(got["wtc"][c], s["wtc"][c])
        assert not got["cam_keep"][c]
    assert np.array_equal(got["point"][e["invalid_track"]], s["point"][e["invalid_track"]])
    bt = e["behind_track"]  # participates, never moves (its factors are behind the cameras), dropped for cheirality
    assert np.array_equal(got["point"][bt], s["point"][bt]) and not got["track_keep"][bt]
    assert not got["track_keep"][list(e["invalid_cam_tracks"])].any() and not got["track_keep"][e["invalid_track"]]
    assert got["stats"][6] == 12 and got["stats"][7] == 299


def test_two_calls_give_identical_bytes():
    s, _, got = _case("medium", 6, True)
    again = _gpu(s, robust=True, reproj_error_thresh=THRESH)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k


def test_float32_uv_no_masks_and_device_track_count():
    """The upstream layout: float32 uv, NULL masks, and the track count read on the device."""
    from gtsfm_amd import device

    s = ref.scene_small(1)
    uv32 = s["uv"].astype(np.float32)
    s32 = dict(s, uv=uv32.astype(np.float64))
    want = ref.global_ba_ref(s["offsets"][:31], s["img"][:s["offsets"][30]], s32["uv"][:s["offsets"][30]],
                             s["point"][:30], None, None, s["wRc"], s["wtc"], s["intr"], None, robust=True,
                             reproj_error_thresh=THRESH)
    r = device.global_ba(_t(s["offsets"], np.int32), _t(s["img"], np.int32), _t(uv32), _t(s["point"]), None, None,
                         _t(s["wRc"]), _t(s["wtc"]), _t(s["intr"]), None, robust=True, reproj_error_thresh=THRESH,
                         n_tracks_dev=torch.tensor([30], dtype=torch.int64, device=DEV))
    stats = r.stats.cpu().numpy()
    _counts_equal(stats, want.stats, "float32 uv")
    np.testing.assert_array_equal(stats[6:], want.stats[6:])
    np.testing.assert_array_equal(r.track_keep.cpu().numpy()[:30], want.track_keep)
    assert not r.track_keep.cpu().numpy()[30:].any()
    assert np.array_equal(r.point.cpu().numpy()[30:], s["point"][30:])
    assert np.abs(r.point.cpu().numpy()[:30] - want.point).max() <= TOL["point"] * np.abs(want.point).max()


def test_pcg_cap_is_counted_and_outputs_stay_consistent():
    s = ref.scene_small(1)
    want = ref.global_ba_ref(*ref.call_args(s), robust=True, reproj_error_thresh=THRESH, pcg_max_iter=3)
    got = _gpu(s, robust=True, reproj_error_thresh=THRESH, pcg_max_iter=3)
    print("cap 3: gpu", got["stats"].tolist(), "ref", want.stats.tolist())
    assert got["stats"][5] > 0 and want.stats[5] > 0
    assert got["stats"][4] <= 3 * got["stats"][3]  # at most 3 products per trial
    assert all(np.isfinite(got[k]).all() for k in ("wRc", "wtc", "point", "stats"))
    assert got["stats"][1] <= got["stats"][0]  # every accepted step lowered the error
    assert got["stats"][8] == got["track_keep"].sum() and got["stats"][9] == 0
    for c in range(5):
        np.testing.assert_allclose(got["wRc"][c] @ got["wRc"][c].T, np.eye(3), atol=1e-12)


def test_empty_problem_is_the_early_return():
    s = ref.scene_small(1)
    for change in (dict(track_valid=np.zeros(40, np.uint8)), dict(cam_valid=np.zeros(5, np.uint8)),
                   dict(meas_valid=np.zeros(len(s["img"]), np.uint8))):
        got = _gpu(dict(s, **change), robust=True, reproj_error_thresh=THRESH)
        assert got["stats"].tolist() == [0.0] * 9 + [1.0]
        assert not got["track_keep"].any() and not got["cam_keep"].any()
        assert np.array_equal(got["wRc"], s["wRc"]) and np.array_equal(got["wtc"], s["wtc"])
        assert np.array_equal(got["point"], s["point"])


def test_argument_errors():
    from gtsfm_amd import device, native

    s = ref.scene_small(1)
    for bad in (dict(measurement_sigma=0.0), dict(cam_pose3_prior_sigma=-1.0), dict(max_iterations=-1),
                dict(pcg_rel_tol=0.0), dict(pcg_max_iter=0), dict(reproj_error_thresh=0.0),
                dict(reproj_error_thresh=float("nan"))):
        with pytest.raises(native.NativeError, match=f"status {native.GTSFM_ERR_ARG}"):
            _gpu(s, **bad)
    with pytest.raises(native.NativeError, match=f"status {native.GTSFM_ERR_CAPACITY}"):
        _gpu(s, workspace_bytes=1024)
    L = native.lib()
    rc = L.gtsfm_global_ba(None, None, None, 0, 40, None, 100, None, None, None, None, None, None, None, 5, 0, 1.0,
                           0.1, 0, 1e-10, 2000, 3.0, None, 0, None, None, None, None, None, None, None)
    assert rc == native.GTSFM_ERR_ARG


# ---------------------------------------------------------------- real data: the door fixture, from the triangulation
@functools.lru_cache(maxsize=None)
def _door():
    from gtsfm_amd.bundle.global_ba import GlobalBundleAdjustment
    from gtsfm_amd.common import geometry as g
    from gtsfm_amd.data_association.data_assoc import DataAssociation
    from gtsfm_amd.data_association.dsf_tracks_estimator import Tracks2d
    from gtsfm_amd.data_association.point3d_initializer import TriangulationOptions, TriangulationSamplingMode

    off, img, uv, cams = triangulation_ref.load_door()
    n = len(cams.wRc)
    f, u0, v0 = cams.intr[0]
    gt = {i: g.PinholeCameraCal3Bundler(g.Pose3(g.Rot3(cams.wRc[i]), cams.wtc[i]), g.Cal3Bundler(f, 0, 0, u0, v0))
          for i in range(n)}
    tracks = Tracks2d(_t(off, np.int32), _t(img, np.int32), None, _t(uv), None)
    da = DataAssociation(2, TriangulationOptions(TriangulationSamplingMode.NO_RANSAC, reproj_error_threshold=5.0))
    tri, valid = da.run_triangulation_arrays(gt, tracks)
    rng = np.random.default_rng(0)
    baseline = np.mean([np.linalg.norm(cams.wtc[i + 1] - cams.wtc[i]) for i in range(n - 1)])
    axis = rng.normal(size=(n, 3))
    xi = np.concatenate([np.radians(0.5) * axis / np.linalg.norm(axis, axis=1, keepdims=True),
                         0.01 * baseline * rng.normal(size=(n, 3))], 1)
    R0, t0 = ref.pose_retract(cams.wRc, cams.wtc, xi)
    pert = (_t(R0), _t(t0), _t(cams.intr), _t(np.ones(n, np.uint8)))
    ba = GlobalBundleAdjustment(robust_measurement_noise=True, max_iterations=10)
    out = ba.run_ba_arrays(pert, tracks, tri, valid, reproj_error_thresh=THRESH)
    got = {k: getattr(out, k).cpu().numpy() for k in ("wRc", "wtc", "point", "track_keep", "cam_keep", "stats")}
    s = dict(offsets=off, img=img, uv=uv.astype(np.float64), point=tri.point.cpu().numpy(),
             track_valid=valid.cpu().numpy().astype(np.uint8), meas_valid=tri.inlier.cpu().numpy(), wRc=R0, wtc=t0,
             intr=cams.intr, cam_valid=np.ones(n, np.uint8))
    want = ref.global_ba_ref(*ref.call_args(s), robust=True, max_iterations=10, reproj_error_thresh=THRESH)
    return s, cams, want, got


def test_door_fixture_from_the_triangulation():
    s, cams, want, got = _door()
    print(f"door: {int(got['stats'][7])} tracks on {int(got['stats'][6])} cameras, PCG iterations "
          f"{got['stats'][4]:.0f} over {got['stats'][3]:.0f} trials")
    _compare("door", s, want, got)
    assert got["stats"][1] < got["stats"][0]
    n = len(cams.wRc)
    for i in range(n):
        for j in range(i + 1, n):
            gt = cams.wRc[i].T @ cams.wRc[j]
            before = ref.rel_rot_deg(gt, s["wRc"][i].T @ s["wRc"][j])
            after = ref.rel_rot_deg(gt, got["wRc"][i].T @ got["wRc"][j])
            assert after < before, f"pair ({i}, {j}): {after:.4f} deg after, {before:.4f} deg before"
