"""gtsfm_global_ba_calib on the MI355X against its restatement (tests/global_ba_calib_ref.py).

Scenes: global_ba_ref's ring scenes, their ground truth re-projected by a camera with k1 = -0.3, k2 = 0.05 (one to two
pixels at the edge of these scenes), the initial calibration f off by 3 % with k1 = k2 = 0:
  small    5 cameras x 40 points: everything inside one wave;
  medium   12 (+2) cameras x 300 points with scene_medium's edge entries (an invalid camera, an unseen camera, an invalid
           track, a measurement switched off, a landmark behind its cameras);
  medium0  medium with camera 0 invalid too and a principal point that differs per camera: the shared variable must come
           from camera 1;
  dense    3 cameras x 400 points: 400 measurements per camera, past a camera workgroup's 256 lanes.
The seeds leave the restatement a decision margin above 1e-6 on every configuration (tests/test_global_ba_calib.py
checks that on the CPU), so LM iterations, trials, keep masks and counters must equal the restatement's.

Tolerances. MEASURED is the largest difference between the restatement and itself with every per-camera sum taken in
the reverse order, over CONFIGS (tests/test_global_ba_calib.py recomputes it): what a different summation order changes,
measured on the reference alone. TOL is ten times that, capped by the project's ceilings (1e-4 degrees; 1e-6 relative
for translations, points, errors and f; 1e-6 absolute for k1, k2).
"""
import functools

import numpy as np
import pytest
import torch

import global_ba_calib_ref as cref
import global_ba_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
THRESH = 3.0
LOOSE, TIGHT = 50.0, 1e-5
# (scene, seed, robust, shared_calib, calibration_prior_sigma)
CONFIGS = (("small", 2, True, False, LOOSE), ("medium", 6, True, False, LOOSE), ("medium", 10, False, False, LOOSE),
           ("medium0", 1, True, True, LOOSE), ("dense", 3, True, True, LOOSE), ("dense", 3, True, False, LOOSE),
           ("medium", 6, True, False, TIGHT), ("medium0", 1, True, True, TIGHT))
IMPROVES = ("medium", 6, True, False, LOOSE)
CHAIN = ("medium", 6)  # per camera, robust, loose prior, thresholds 10, 5, 3
CHAIN_THRESHOLDS = [10, 5, 3]
#  rotation (deg); translation, points, error, f relative; k1, k2 absolute
MEASURED = dict(rot=1.1e-9, trans=2.0e-11, point=8.2e-10, err=7.7e-13, f=1.7e-11, k=6.3e-8)
TOL = {k: 10.0 * v for k, v in MEASURED.items()}
CEILING = dict(rot=1e-4, trans=1e-6, point=1e-6, err=1e-6, f=1e-6, k=1e-6)
assert all(TOL[k] <= CEILING[k] for k in TOL)
OUT = ("wRc", "wtc", "point", "track_keep", "cam_keep", "stats", "calib")


def modelled_cameras(s):
    """The cameras the medium scenes model: valid and seen by a measurement (every such camera has a usable one)."""
    return np.nonzero(np.asarray(s["cam_valid"], bool) & np.isin(np.arange(len(s["calib"])), s["img"]))[0]


def differences(s, got, want):
    """rot (deg), trans, point, err, f (relative) and k (absolute) between a result dict and a restatement result."""
    cams = modelled_cameras(s)
    rot, tr = ref.pose_diff(got["wRc"], got["wtc"], want.wRc, want.wtc, cams)
    dp = np.abs(got["point"] - want.point).max() / np.abs(want.point).max()
    de = max(abs(got["stats"][k] - want.stats[k]) / max(abs(want.stats[k]), 1e-300) for k in (0, 1))
    df, dk = cref.calib_diff(got["calib"], want.calib, cams)
    return dict(rot=rot, trans=tr, point=dp, err=de, f=df, k=dk)


def chain_ref(s):
    """The restatement's three stages: each from the initial poses and landmarks and the calibration before it."""
    rounds, calib = [], s["calib"]
    for th in CHAIN_THRESHOLDS:
        rounds.append(cref.global_ba_calib_ref(*cref.call_args(dict(s, calib=calib)), robust=True, shared_calib=False,
                                               calibration_prior_sigma=LOOSE, reproj_error_thresh=float(th)))
        calib = rounds[-1].calib
    return rounds


def _t(a, dtype=None):
    if a is None:
        return None
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))
    return torch.from_numpy(a).to(DEV)


def _gpu(s, **kw):
    from gtsfm_amd import device

    r = device.global_ba_calib(_t(s["offsets"], np.int32), _t(s["img"], np.int32), _t(s["uv"]), _t(s["point"]),
                               _t(s["track_valid"], np.uint8), _t(s["meas_valid"], np.uint8), _t(s["wRc"]),
                               _t(s["wtc"]), _t(s["calib"]), _t(s["cam_valid"], np.uint8), **kw)
    return {k: getattr(r, k).cpu().numpy() for k in OUT}


@functools.lru_cache(maxsize=None)
def _case(name, seed, robust, shared, sigma):
    s = cref.SCENES[name](seed)
    kw = dict(robust=robust, shared_calib=shared, calibration_prior_sigma=sigma, reproj_error_thresh=THRESH)
    return s, cref.global_ba_calib_ref(*cref.call_args(s), **kw), _gpu(s, **kw)


def _compare(label, s, want, got):
    """Counts and masks equal, PCG total within 2 per trial; poses, points, errors and calibration within TOL. Prints
    every figure before asserting."""
    d = differences(s, got, want)
    print(f"{label}: " + ", ".join(f"{k} {v:.3e}" for k, v in d.items()) + f"; stats gpu {got['stats'].tolist()} ref "
          f"{want.stats.tolist()}; ref margin {want.min_margin:.2e}")
    assert want.min_margin > 1e-6  # the seeds are chosen for it (tests/test_global_ba_calib.py)
    np.testing.assert_array_equal(got["stats"][[2, 3, 5]], want.stats[[2, 3, 5]], err_msg=label)
    assert abs(got["stats"][4] - want.stats[4]) <= 2 * want.stats[3], f"{label}: PCG iterations"
    np.testing.assert_array_equal(got["stats"][6:11], want.stats[6:11], err_msg=label)
    np.testing.assert_array_equal(got["track_keep"], want.track_keep, err_msg=label)
    np.testing.assert_array_equal(got["cam_keep"], want.cam_keep, err_msg=label)
    assert abs(got["stats"][11] - want.stats[11]) <= TOL["f"] * 2
    for k in d:
        assert d[k] <= TOL[k], f"{label}: {k} {d[k]:.3e} > {TOL[k]:.3e}"


@pytest.mark.parametrize("name,seed,robust,shared,sigma", CONFIGS)
def test_matches_restatement(name, seed, robust, shared, sigma):
    s, want, got = _case(name, seed, robust, shared, sigma)
    _compare(f"{name} robust={robust} shared={shared} sigma={sigma}", s, want, got)
    assert got["stats"][1] < got["stats"][0] and got["stats"][9] == 0


def test_refinement_improves_the_fit():
    """Loose prior on medium: every modelled camera's f moves towards the truth, and the fit is better than
    device.global_ba reaches on the same inputs with the distortion dropped from the model."""
    from gtsfm_amd import device

    s, want, got = _case(*IMPROVES)
    cams = modelled_cameras(s)
    f_true = s["gt_calib"][cams, 0]
    print("f refined", got["calib"][cams, 0].tolist())
    assert (np.abs(got["calib"][cams, 0] - f_true) < np.abs(s["calib"][cams, 0] - f_true)).all()
    a = cref.undistorted_args(s)
    fixed = device.global_ba(_t(a[0], np.int32), _t(a[1], np.int32), _t(a[2]), _t(a[3]), _t(a[4], np.uint8),
                             _t(a[5], np.uint8), _t(a[6]), _t(a[7]), _t(np.ascontiguousarray(a[8])),
                             _t(a[9], np.uint8), robust=IMPROVES[2], reproj_error_thresh=THRESH)
    fixed_err = fixed.stats.cpu().numpy()[1]
    print(f"final error refined {got['stats'][1]:.3f}, fixed {fixed_err:.3f}")
    assert got["stats"][1] < fixed_err


@pytest.mark.parametrize("cfg", (CONFIGS[1], CONFIGS[3]))
def test_non_entries_are_the_inputs_bit_for_bit(cfg):
    s, want, got = _case(*cfg)
    e = s["edge"]
    cams = modelled_cameras(s)
    for c in sorted(set(range(len(s["calib"]))) - set(cams.tolist())):
        assert np.array_equal(got["wRc"][c], s["wRc"][c]) and np.array_equal(got["wtc"][c], s["wtc"][c])
        assert np.array_equal(got["calib"][c], s["calib"][c]) and not got["cam_keep"][c]
    assert {e["invalid_cam"], e["unseen_cam"]} <= set(range(len(s["calib"]))) - set(cams.tolist())
    assert np.array_equal(got["point"][e["invalid_track"]], s["point"][e["invalid_track"]])
    bt = e["behind_track"]  # participates, never moves (its factors are behind the cameras), dropped for cheirality
    assert np.array_equal(got["point"][bt], s["point"][bt]) and not got["track_keep"][bt]
    # u0, v0 are no variables
    shared = cfg[3]
    if not shared:
        assert np.array_equal(got["calib"][cams, 3:], s["calib"][cams, 3:])
        assert got["stats"][10] == len(cams) == 12
    else:
        c0 = cams[0]
        assert c0 == 1 and got["stats"][10] == 1 and len(cams) == 11
        assert (got["calib"][cams] == got["calib"][c0]).all()  # one calibration, bit for bit, in every modelled row
        assert np.array_equal(got["calib"][c0, 3:], s["calib"][c0, 3:])  # the lowest modelled camera's u0, v0
        assert not np.array_equal(s["calib"][c0, 3:], s["calib"][cams[1], 3:])


@pytest.mark.parametrize("cfg", (CONFIGS[1], CONFIGS[3]))
def test_two_calls_give_identical_bytes(cfg):
    s, _, got = _case(*cfg)
    again = _gpu(s, robust=cfg[2], shared_calib=cfg[3], calibration_prior_sigma=cfg[4], reproj_error_thresh=THRESH)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k


def test_argument_errors_and_empty_problem():
    from gtsfm_amd import native

    s = cref.scene_small(2)
    for bad in (dict(calibration_prior_sigma=0.0), dict(calibration_prior_sigma=-1.0),
                dict(calibration_prior_sigma=float("nan")), dict(measurement_sigma=0.0), dict(pcg_max_iter=0)):
        with pytest.raises(native.NativeError, match=f"status {native.GTSFM_ERR_ARG}"):
            _gpu(s, **bad)
    with pytest.raises(native.NativeError, match=f"status {native.GTSFM_ERR_CAPACITY}"):
        _gpu(s, workspace_bytes=1024)
    L = native.lib()
    base = [None, None, None, 0, 40, None, 100, None, None, None, None, None, None, None, 5, 0, 1.0, 0.1]
    tail = [0, 1e-10, 2000, 3.0, None, 0, None, None, None, None, None, None, None, None]
    assert L.gtsfm_global_ba_calib(*base, 2, 1.0, *tail) == native.GTSFM_ERR_ARG  # shared_calib outside {0, 1}
    for change in (dict(track_valid=np.zeros(40, np.uint8)), dict(cam_valid=np.zeros(5, np.uint8)),
                   dict(meas_valid=np.zeros(len(s["img"]), np.uint8))):
        for shared in (False, True):
            got = _gpu(dict(s, **change), robust=True, shared_calib=shared, calibration_prior_sigma=LOOSE,
                       reproj_error_thresh=THRESH)
            assert got["stats"].tolist() == [0.0] * 9 + [1.0, 0.0, 0.0]
            assert not got["track_keep"].any() and not got["cam_keep"].any()
            assert np.array_equal(got["wRc"], s["wRc"]) and np.array_equal(got["wtc"], s["wtc"])
            assert np.array_equal(got["point"], s["point"]) and np.array_equal(got["calib"], s["calib"])
    # an empty shape (tracks without a single measurement): status 1 before the workspace is looked at
    from gtsfm_amd import device

    r = device.global_ba_calib(_t(np.zeros(41, np.int32)), _t(np.zeros(0, np.int32)), _t(np.zeros((0, 2))),
                               _t(s["point"]), None, None, _t(s["wRc"]), _t(s["wtc"]), _t(s["calib"]), None,
                               calibration_prior_sigma=LOOSE, workspace_bytes=0)
    assert r.stats.cpu().numpy().tolist() == [0.0] * 9 + [1.0, 0.0, 0.0]
    assert np.array_equal(r.calib.cpu().numpy(), s["calib"]) and np.array_equal(r.point.cpu().numpy(), s["point"])


def test_three_stages_through_the_optimizer():
    """BundleAdjustmentOptimizer(refine_calibration=True, reproj_error_thresholds=[10, 5, 3]).run_ba_arrays: three
    calls, each from the calibration the one before refined; equal to three chained restatement calls."""
    from gtsfm_amd import device
    from gtsfm_amd.bundle.bundle_adjustment import BundleAdjustmentOptimizer
    from gtsfm_amd.data_association.dsf_tracks_estimator import Tracks2d
    from gtsfm_amd.data_association.point3d_initializer import Triangulated

    s = cref.SCENES[CHAIN[0]](CHAIN[1])
    rounds = chain_ref(s)
    seen = []
    inner = device.global_ba_calib

    def spy(*args, **kw):
        seen.append((args[8].cpu().numpy().copy(), kw["reproj_error_thresh"]))
        return inner(*args, **kw)

    T = len(s["offsets"]) - 1
    tracks = Tracks2d(_t(s["offsets"], np.int32), _t(s["img"], np.int32), None, _t(s["uv"]), None)
    fields = dict(exit_code=torch.zeros(T, dtype=torch.int32, device=DEV), point=_t(s["point"]),
                  inlier=_t(s["meas_valid"], np.uint8))
    tri = Triangulated(**{k: fields.get(k) for k in Triangulated._fields})
    cams = (_t(s["wRc"]), _t(s["wtc"]), _t(s["calib"]), _t(s["cam_valid"], np.uint8))
    ba = BundleAdjustmentOptimizer(reproj_error_thresholds=CHAIN_THRESHOLDS, robust_measurement_noise=True,
                                   calibration_prior_noise_sigma=LOOSE, refine_calibration=True)
    device.global_ba_calib = spy
    try:
        out = ba.run_ba_arrays(cams, tracks, tri, _t(s["track_valid"], np.uint8))
    finally:
        device.global_ba_calib = inner
    assert [th for _, th in seen] == [10.0, 5.0, 3.0]
    assert np.array_equal(seen[0][0], s["calib"])
    cams_m = modelled_cameras(s)
    for k in (1, 2):  # stage k starts from stage k - 1's refined calibration
        df, dk = cref.calib_diff(seen[k][0], rounds[k - 1].calib, cams_m)
        print(f"stage {k} input: df/f {df:.3e}, dk {dk:.3e}")
        assert df <= TOL["f"] and dk <= TOL["k"] and not np.array_equal(seen[k][0], seen[k - 1][0])
    got = {k: getattr(out, k).cpu().numpy() for k in OUT}
    _compare("three stages", s, rounds[-1], got)
