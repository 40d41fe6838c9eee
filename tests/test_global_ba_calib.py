"""Self-calibrating global bundle adjustment without a GPU: the numpy restatement (tests/global_ba_calib_ref.py) against
finite differences, against the fixed-calibration restatement in the limit of a tight prior, against itself with its
per-camera sums reversed, and the Python layer with the native call replaced by the restatement.

FIXED_LIMIT_MEASURED holds what test_fixed_calibration_is_the_limit_of_a_tight_prior measured (sigma 1e-5, undistorted
scenes): the fixed-calibration call is the limit of this one, far inside the GPU ceilings of 1e-4 degrees and 1e-6.
The summation-order figures are in tests/test_global_ba_calib_gpu.py (MEASURED), where they set the GPU tolerances; this
file checks that they are what the restatement gives.
"""
import functools

import numpy as np
import pytest

import global_ba_calib_ref as cref
import global_ba_ref as ref
from test_global_ba_calib_gpu import (CEILING, CHAIN, CONFIGS, IMPROVES, MEASURED, THRESH, TOL, chain_ref, differences,
                                      modelled_cameras)

MIN_MARGIN = 1e-6
#                            rotation (deg), translation, points, error (relative)
FIXED_LIMIT_MEASURED = dict(rot=2e-10, trans=2e-11, point=4e-11, err=1e-11)  # seen: 1.3e-10, 1.2e-11, 2.4e-11, 5.6e-12


@functools.lru_cache(maxsize=None)
def solve(name, seed, robust, shared, sigma, reverse=False):
    s = cref.SCENES[name](seed)
    return s, cref.global_ba_calib_ref(*cref.call_args(s), robust=robust, shared_calib=shared,
                                       calibration_prior_sigma=sigma, reproj_error_thresh=THRESH,
                                       reverse_cam_order=reverse)


def test_jacobians_against_central_differences():
    rng = np.random.default_rng(0)
    s = cref.scene_small(1)
    n = 20
    c = s["img"][:n]
    R, t = s["gt_wRc"][c], s["gt_wtc"][c]
    K = s["gt_calib"][c] + np.array([0.0, 0.0, 0.0, 0.0, 0.0])
    p = s["gt_point"][np.repeat(np.arange(40), np.diff(s["offsets"]))[:n]] + rng.normal(0, 0.05, (n, 3))
    pc, _, ok = cref.project_k(R, t, K, p)
    assert ok.all() and np.abs(K[:, 1]).min() > 0 and np.abs(K[:, 2]).min() > 0  # distortion is on
    Jp, Jx, Jk = cref.reproj_jacobians_k(R, t, K, pc)
    h = 1e-5
    Np, Nx, Nk = np.zeros_like(Jp), np.zeros_like(Jx), np.zeros_like(Jk)
    for k in range(3):
        d = np.zeros(3)
        d[k] = h
        Np[:, :, k] = (cref.project_k(R, t, K, p + d)[1] - cref.project_k(R, t, K, p - d)[1]) / (2 * h)
        dk = np.zeros(5)
        dk[k] = h * (100.0 if k == 0 else 1.0)  # f is O(1000)
        Nk[:, :, k] = (cref.project_k(R, t, K + dk, p)[1] - cref.project_k(R, t, K - dk, p)[1]) / (2 * dk[k])
    for k in range(6):
        xi = np.zeros((n, 6))
        xi[:, k] = h
        Rp, tp = ref.pose_retract(R, t, xi)
        Rm, tm = ref.pose_retract(R, t, -xi)
        Nx[:, :, k] = (cref.project_k(Rp, tp, K, p)[1] - cref.project_k(Rm, tm, K, p)[1]) / (2 * h)
    # the bar is relative to the largest entry of each block; the columns of Jk differ by orders of magnitude
    assert np.abs(Jp - Np).max() / np.abs(Jp).max() < 1e-6
    assert np.abs(Jx - Nx).max() / np.abs(Jx).max() < 1e-6
    for k in range(3):
        assert np.abs(Jk[:, :, k] - Nk[:, :, k]).max() / np.abs(Jk[:, :, k]).max() < 1e-6, k
    # and the distorted Jacobians are not the pinhole ones
    Jp0, _ = ref.reproj_jacobians(R, t, K[:, [0, 3, 4]], pc)
    assert np.abs(Jp - Jp0).max() / np.abs(Jp).max() > 1e-3


@pytest.mark.parametrize("name,fn,seed,shared", (("small", ref.scene_small, 1, False),
                                                 ("medium", ref.scene_medium, 6, False),
                                                 ("medium", ref.scene_medium, 6, True)))
def test_fixed_calibration_is_the_limit_of_a_tight_prior(name, fn, seed, shared):
    """Undistorted scene, sigma 1e-5: poses, points and error are global_ba_ref's."""
    s = fn(seed)
    calib = np.concatenate([s["intr"][:, :1], np.zeros((len(s["intr"]), 2)), s["intr"][:, 1:]], 1)
    a = ref.global_ba_ref(*ref.call_args(s), robust=True, reproj_error_thresh=THRESH)
    b = cref.global_ba_calib_ref(*ref.call_args(s)[:8], calib, s["cam_valid"], robust=True, shared_calib=shared,
                                 calibration_prior_sigma=1e-5, reproj_error_thresh=THRESH)
    cams = np.nonzero(a.cam_keep)[0]
    rot, tr = ref.pose_diff(b.wRc, b.wtc, a.wRc, a.wtc, cams)
    dp = np.abs(b.point - a.point).max() / np.abs(a.point).max()
    de = abs(b.stats[1] - a.stats[1]) / a.stats[1]
    df, dk = cref.calib_diff(b.calib, calib, cams)
    print(f"{name} shared={shared}: rot {rot:.2e} deg, trans {tr:.2e}, point {dp:.2e}, error {de:.2e}; calibration "
          f"moved by df/f {df:.2e}, dk {dk:.2e}")
    np.testing.assert_array_equal(a.stats[[2, 3, 6, 7, 8]], b.stats[[2, 3, 6, 7, 8]])
    np.testing.assert_array_equal(a.track_keep, b.track_keep)
    assert rot < 1e-4 and tr < 1e-6 and dp < 1e-6 and de < 1e-6
    got = dict(rot=rot, trans=tr, point=dp, err=de)
    assert all(got[k] <= FIXED_LIMIT_MEASURED[k] for k in got), got


@pytest.mark.parametrize("name,seed,robust,shared,sigma", CONFIGS)
def test_seeds_leave_a_decision_margin(name, seed, robust, shared, sigma):
    _, r = solve(name, seed, robust, shared, sigma)
    assert r.min_margin > MIN_MARGIN, f"{name} seed {seed}: margin {r.min_margin:.2e}"
    assert r.stats[1] < r.stats[0] and r.stats[5] == 0


def test_chained_stages_leave_a_decision_margin():
    s = cref.SCENES[CHAIN[0]](CHAIN[1])
    rounds = chain_ref(s)
    assert len(rounds) == 3 and all(r.min_margin > MIN_MARGIN for r in rounds), [r.min_margin for r in rounds]
    # each stage starts from the calibration before it: its prior cost starts at zero, its f differs from the input's
    assert not np.array_equal(rounds[0].calib, rounds[1].calib)


def test_summation_order_sensitivity_is_what_the_gpu_file_records():
    """The restatement with its per-camera sums reversed: the largest differences over the GPU configurations are the
    MEASURED of tests/test_global_ba_calib_gpu.py (recorded with a little headroom: not above twice what is seen here),
    and ten times them stays under the project's ceilings."""
    worst = dict.fromkeys(MEASURED, 0.0)
    for name, seed, robust, shared, sigma in CONFIGS:
        s, a = solve(name, seed, robust, shared, sigma)
        _, b = solve(name, seed, robust, shared, sigma, True)
        np.testing.assert_array_equal(a.stats[[2, 3, 5, 6, 7, 8, 10]], b.stats[[2, 3, 5, 6, 7, 8, 10]])
        d = differences(s, dict(wRc=b.wRc, wtc=b.wtc, point=b.point, stats=b.stats, calib=b.calib), a)
        print(name, seed, robust, shared, sigma, {k: f"{v:.2e}" for k, v in d.items()})
        worst = {k: max(worst[k], d[k]) for k in worst}
    print("worst", {k: f"{v:.2e}" for k, v in worst.items()})
    for k in worst:
        assert worst[k] <= MEASURED[k] <= max(2.0 * worst[k], 1e-15), (k, worst[k], MEASURED[k])
        assert TOL[k] == 10.0 * MEASURED[k] and TOL[k] <= CEILING[k], k


def test_refinement_improves_the_fit_on_the_restatement():
    """The two conditions tests/test_global_ba_calib_gpu.py::test_refinement_improves_the_fit relies on."""
    name, seed, robust, shared, sigma = IMPROVES
    s, r = solve(name, seed, robust, shared, sigma)
    cams = modelled_cameras(s)
    f_true = s["gt_calib"][cams, 0]
    assert (np.abs(r.calib[cams, 0] - f_true) < np.abs(s["calib"][cams, 0] - f_true)).all()
    fixed = ref.global_ba_ref(*cref.undistorted_args(s), robust=robust, reproj_error_thresh=THRESH)
    print(f"final error refined {r.stats[1]:.3f}, fixed {fixed.stats[1]:.3f}; distortion {s['distortion_px']:.2f} px")
    assert r.stats[1] < fixed.stats[1]
    assert s["distortion_px"] > 1.0


def test_shared_mode_takes_the_first_modelled_camera():
    s, r = solve("medium0", 1, True, True, 50.0)
    cams = modelled_cameras(s)
    assert cams[0] == 1 and not s["cam_valid"][0]
    assert (r.calib[cams] == r.calib[1]).all() and np.array_equal(r.calib[1, 3:], s["calib"][1, 3:])
    assert not np.array_equal(s["calib"][1, 3:], s["calib"][2, 3:])
    e = s["edge"]
    for c in (0, e["invalid_cam"], e["unseen_cam"]):  # not modelled: copied through
        assert np.array_equal(r.calib[c], s["calib"][c]) and np.array_equal(r.wRc[c], s["wRc"][c])
    assert r.stats[10] == 1 and r.stats[6] == 11


# ---------------------------------------------------------------- the Python layer, with the native calls replaced
def _ba_data(s):
    from gtsfm_amd.bundle.bundle_adjustment import BaData
    from gtsfm_amd.common import geometry as g
    from gtsfm_amd.common.sfm_track import SfmTrack

    cams = {i: g.PinholeCameraCal3Bundler(g.Pose3(g.Rot3(s["wRc"][i]), s["wtc"][i]), g.Cal3Bundler(*s["calib"][i]))
            for i in range(len(s["calib"]))}
    tracks = []
    for j in range(len(s["offsets"]) - 1):
        t = SfmTrack(s["point"][j])
        for m in range(s["offsets"][j], s["offsets"][j + 1]):
            t.addMeasurement(int(s["img"][m]), s["uv"][m])
        tracks.append(t)
    return BaData(cams, tracks)


@pytest.fixture
def restated_kernels(monkeypatch):
    """device.global_ba and device.global_ba_calib answered by the restatements on CPU tensors."""
    import torch

    from gtsfm_amd import device, native
    from gtsfm_amd.common import upload

    calls = []

    def arrays(args):
        return [None if x is None else x.numpy() for x in args]

    def tensors(xs):
        return (torch.from_numpy(np.ascontiguousarray(x)) for x in xs)

    def fake_fixed(*args, **kw):
        calls.append(("global_ba", dict(kw)))
        r = ref.global_ba_ref(*arrays(args), robust=kw["robust"], reproj_error_thresh=kw["reproj_error_thresh"])
        return device.GlobalBaResult(*tensors(r[:6]))

    def fake_calib(*args, **kw):
        calls.append(("global_ba_calib", dict(kw), args[8].numpy().copy()))
        r = cref.global_ba_calib_ref(*arrays(args), robust=kw["robust"], shared_calib=kw["shared_calib"],
                                     calibration_prior_sigma=kw["calibration_prior_sigma"],
                                     reproj_error_thresh=kw["reproj_error_thresh"])
        return device.GlobalBaCalibResult(*tensors(r[:6]), *tensors([r.calib]))

    monkeypatch.setattr(device, "global_ba", fake_fixed)
    monkeypatch.setattr(device, "global_ba_calib", fake_calib)
    monkeypatch.setattr(native, "require_gpu", lambda: None)
    monkeypatch.setattr(upload, "cuda_device", lambda like=None: torch.device("cpu"))
    return calls


def test_off_is_todays_behaviour(restated_kernels):
    from gtsfm_amd.bundle.bundle_adjustment import BaData, BundleAdjustmentOptimizer
    from gtsfm_amd.common import geometry as g

    s = cref.scene_small(2)
    data = _ba_data(s)  # k1 = k2 = 0 initially
    ba = BundleAdjustmentOptimizer(reproj_error_thresholds=[10, 3], shared_calib=True,
                                   calibration_prior_noise_sigma=50.0)
    opt, _, _ = ba.run_ba(data, [], {})
    assert [c[0] for c in restated_kernels] == ["global_ba"]  # one call, the fixed-calibration one
    assert restated_kernels[0][1]["reproj_error_thresh"] == 3.0
    assert opt.calibrations is None
    assert np.array_equal(g.calibration_params5(opt.cameras[0].calibration()), s["calib"][0])
    cams = dict(data.cameras)
    cams[0] = g.PinholeCameraCal3Bundler(cams[0].pose(), g.Cal3Bundler(1000, 0.1, 0, 500, 400))
    with pytest.raises(NotImplementedError, match="radial distortion.*refine_calibration=True"):
        ba.run_ba(BaData(cams, data.tracks), [], {})


@pytest.mark.parametrize("shared", (False, True))
def test_on_goes_through_global_ba_calib(restated_kernels, shared):
    from gtsfm_amd.bundle.bundle_adjustment import BaData
    from gtsfm_amd.bundle.global_ba import GlobalBundleAdjustment
    from gtsfm_amd.common import geometry as g

    s = cref.scene_small(2)
    data = _ba_data(s)
    cams = dict(data.cameras)  # a distorted input camera is accepted
    cams[1] = g.PinholeCameraCal3Bundler(cams[1].pose(), g.Cal3Bundler(1030, -0.01, 0.001, 500, 400))
    data = BaData(cams, data.tracks)
    ba = GlobalBundleAdjustment(reproj_error_thresholds=[10, 3], robust_measurement_noise=True, shared_calib=shared,
                                calibration_prior_noise_sigma=50.0, refine_calibration=True)
    opt, fil, mask = ba.run_ba(data, [], {})
    assert [c[0] for c in restated_kernels] == ["global_ba_calib"] * 2
    for _, kw, _ in restated_kernels:
        assert kw["shared_calib"] is shared and kw["calibration_prior_sigma"] == 50.0 and kw["robust"] is True
    assert [c[1]["reproj_error_thresh"] for c in restated_kernels] == [10.0, 3.0]
    first_in, second_in = restated_kernels[0][2], restated_kernels[1][2]
    assert np.array_equal(first_in[1], [1030, -0.01, 0.001, 500, 400])
    # the second stage starts from what the first refined, which the restatement gives for the first stage alone
    want1 = cref.global_ba_calib_ref(*cref.call_args(dict(s, calib=first_in)), robust=True, shared_calib=shared,
                                     calibration_prior_sigma=50.0, reproj_error_thresh=10.0)
    np.testing.assert_array_equal(second_in, want1.calib)
    want2 = cref.global_ba_calib_ref(*cref.call_args(dict(s, calib=second_in)), robust=True, shared_calib=shared,
                                     calibration_prior_sigma=50.0, reproj_error_thresh=3.0)
    for i, cam in opt.cameras.items():
        cal = cam.calibration()
        assert np.array_equal(g.calibration_params5(cal), want2.calib[i]) and np.array_equal(opt.calibrations[i],
                                                                                             want2.calib[i])
        assert np.array_equal(cam.pose().translation(), want2.wtc[i])
    rows = np.array([g.calibration_params5(c.calibration()) for c in opt.cameras.values()])
    assert (rows == rows[0]).all() if shared else not (rows == rows[0]).all()
    assert mask == [bool(k) for k in want2.track_keep] and len(fil.tracks) == sum(mask)
    assert sorted(fil.calibrations) == sorted(fil.cameras)


def test_calibration_params5_and_result_defaults():
    from gtsfm_amd.bundle.bundle_adjustment import BaArrays, BaData
    from gtsfm_amd.common import geometry as g

    assert g.calibration_params5(g.Cal3Bundler(900, -0.2, 0.03, 320, 240)).tolist() == [900, -0.2, 0.03, 320, 240]
    assert BaData({}, []).calibrations is None and BaArrays(*[None] * 6).calib is None


def test_workspace_query_without_gpu():
    from gtsfm_amd import native

    q = native.lib().gtsfm_global_ba_calib_workspace_bytes
    assert q(14000, 205000, 1000) > 205000 * 208
    assert q(40, 150, 5) > native.lib().gtsfm_global_ba_workspace_bytes(40, 150, 5)
    for shape in ((0, 150, 5), (40, 0, 5), (40, 150, 0), (-1, 150, 5), (2 ** 31, 150, 5), (40, 2 ** 31, 5),
                  (40, 150, 2 ** 20 + 1)):
        assert q(*shape) == 0
