"""Global bundle adjustment without a GPU: the numpy restatement (tests/global_ba_ref.py) against itself and against
ground truth, the filter semantics, the host API's argument handling and the workspace query.

The seeds of the three synthetic scenes are chosen so that the restatement's smallest decision margin exceeds
MIN_MARGIN on each (checked here); tests/test_global_ba_gpu.py asserts equal LM counts on exactly these configurations.
"""
import functools

import numpy as np
import pytest

import global_ba_ref as ref

MIN_MARGIN = 1e-6
THRESH = 3.0
# (name, scene builder, seed, robust): the configurations the GPU test runs
CONFIGS = (("small", ref.scene_small, 1, True), ("medium", ref.scene_medium, 6, True),
           ("medium", ref.scene_medium, 6, False), ("dense", ref.scene_dense, 2, True))


@functools.lru_cache(maxsize=None)
def solve(name, seed, robust, solver="pcg", thresh=THRESH):
    fn = {"small": ref.scene_small, "medium": ref.scene_medium, "dense": ref.scene_dense}[name]
    s = fn(seed)
    return s, ref.global_ba_ref(*ref.call_args(s), robust=robust, reproj_error_thresh=thresh, solver=solver)


def test_jacobians_against_central_differences():
    rng = np.random.default_rng(0)
    s = ref.scene_small(1)
    n = 20
    R, t, K = s["gt_wRc"][s["img"][:n]], s["gt_wtc"][s["img"][:n]], s["intr"][s["img"][:n]]
    p = s["gt_point"][np.repeat(np.arange(40), np.diff(s["offsets"]))[:n]] + rng.normal(0, 0.05, (n, 3))
    pc, _, ok = ref.project(R, t, K, p)
    assert ok.all()
    Jp, Jx = ref.reproj_jacobians(R, t, K, pc)
    h = 1e-5
    Np, Nx = np.zeros_like(Jp), np.zeros_like(Jx)
    for k in range(3):
        d = np.zeros(3)
        d[k] = h
        Np[:, :, k] = (ref.project(R, t, K, p + d)[1] - ref.project(R, t, K, p - d)[1]) / (2 * h)
    for k in range(6):
        xi = np.zeros((n, 6))
        xi[:, k] = h
        Rp, tp = ref.pose_retract(R, t, xi)
        Rm, tm = ref.pose_retract(R, t, -xi)
        Nx[:, :, k] = (ref.project(Rp, tp, K, p)[1] - ref.project(Rm, tm, K, p)[1]) / (2 * h)
    # f = 1000 makes the entries O(1e3); the bar is relative to the largest entry
    assert np.abs(Jp - Np).max() / np.abs(Jp).max() < 1e-6
    assert np.abs(Jx - Nx).max() / np.abs(Jx).max() < 1e-6


def test_pose_prior_residual_is_the_inverse_of_the_retraction():
    rng = np.random.default_rng(1)
    s = ref.scene_small(1)
    xi = rng.normal(0, 0.3, (5, 6))
    R, t = ref.pose_retract(s["gt_wRc"], s["gt_wtc"], xi)
    for c in range(5):
        np.testing.assert_allclose(ref.pose_local(s["gt_wRc"][c], s["gt_wtc"][c], R[c], t[c]), xi[c], atol=1e-12)


@pytest.mark.parametrize("name,fn,seed,robust", CONFIGS)
def test_pcg_follows_exact_cholesky(name, fn, seed, robust):
    _, a = solve(name, seed, robust)
    _, b = solve(name, seed, robust, "exact")
    np.testing.assert_array_equal(a.stats[2:4], b.stats[2:4])  # LM iterations and trials
    np.testing.assert_array_equal(a.track_keep, b.track_keep)
    cams = np.nonzero(a.cam_keep)[0]
    rot, tr = ref.pose_diff(a.wRc, a.wtc, b.wRc, b.wtc, cams)
    print(f"{name} robust={robust}: PCG vs exact {rot:.2e} deg, {tr:.2e} relative translation, "
          f"max PCG iterations per solve {max(a.pcg_iters_per_solve)}, cap hits {a.stats[5]:.0f}")
    assert a.stats[5] == 0 and rot < 1e-8 and tr < 1e-9


@pytest.mark.parametrize("name,fn,seed,robust", CONFIGS)
def test_seeds_leave_a_decision_margin(name, fn, seed, robust):
    for solver in ("pcg", "exact"):
        _, r = solve(name, seed, robust, solver)
        assert r.min_margin > MIN_MARGIN, f"{name} seed {seed} {solver}: margin {r.min_margin:.2e}"


def test_noise_free_scene_recovers_relative_poses():
    s = ref.ring_scene(6, 80, 3, 6, seed=4, noise_px=0.0, outlier_frac=0.0)
    r = ref.global_ba_ref(*ref.call_args(s), robust=False)
    # LM stops on a relative decrease of 1e-5, and the two priors sit at the perturbed camera and landmark (two more
    # constraints than the gauge has freedoms), so the bars are those of a converged LM, not of machine precision
    assert r.stats[1] < 1e-5 * r.stats[0]
    scale = np.linalg.norm(s["gt_wtc"][1] - s["gt_wtc"][0]) / np.linalg.norm(r.wtc[1] - r.wtc[0])
    before = after = 0.0
    for i in range(6):
        for j in range(i + 1, 6):
            gt = s["gt_wRc"][i].T @ s["gt_wRc"][j]
            after = max(after, ref.rel_rot_deg(gt, r.wRc[i].T @ r.wRc[j]))
            before = max(before, ref.rel_rot_deg(gt, s["wRc"][i].T @ s["wRc"][j]))
            gt_t = s["gt_wRc"][i].T @ (s["gt_wtc"][j] - s["gt_wtc"][i])
            got_t = r.wRc[i].T @ (r.wtc[j] - r.wtc[i]) * scale  # relative translations up to the global scale
            assert np.linalg.norm(got_t - gt_t) < 1e-4 * np.linalg.norm(gt_t)
    assert before > 1.0 and after < 1e-3


def _loop_filter(s, r, thresh):
    """GtsfmData.filter_landmarks written track by track, from the restatement's outputs."""
    keep = np.zeros(len(s["offsets"]) - 1, np.uint8)
    worst = np.full(len(keep), np.nan)
    for j in range(len(keep)):
        if not r_part(s, j):
            continue
        ok, errs = True, []
        for m in range(s["offsets"][j], s["offsets"][j + 1]):
            if not s["meas_valid"][m]:
                continue
            c = s["img"][m]
            if not s["cam_valid"][c]:
                ok = False
                continue
            pc = r.wRc[c].T @ (r.point[j] - r.wtc[c])
            if pc[2] <= 0:
                ok = False
                continue
            e = np.linalg.norm(s["intr"][c, 1:] + s["intr"][c, 0] * pc[:2] / pc[2] - s["uv"][m])
            errs.append(e)
            ok = ok and e < thresh
        keep[j] = ok
        worst[j] = max(errs) if ok or errs else np.nan
    return keep, worst


def r_part(s, j):
    m = np.arange(s["offsets"][j], s["offsets"][j + 1])
    usable = s["meas_valid"][m].astype(bool) & s["cam_valid"][s["img"][m]].astype(bool)
    return bool(s["track_valid"][j]) and usable.sum() >= 2


def test_filter_semantics():
    s, r = solve("medium", 6, True)
    keep, worst = _loop_filter(s, r, THRESH)
    np.testing.assert_array_equal(r.track_keep, keep)
    e = s["edge"]
    # the landmark that ends behind a camera, the tracks with a measurement on the invalid camera, the invalid track
    c = s["img"][s["offsets"][e["behind_track"]]]
    assert (r.wRc[c].T @ (r.point[e["behind_track"]] - r.wtc[c]))[2] <= 0 and not r.track_keep[e["behind_track"]]
    assert not r.track_keep[list(e["invalid_cam_tracks"])].any() and not r.track_keep[e["invalid_track"]]
    assert not r.cam_keep[e["invalid_cam"]] and not r.cam_keep[e["unseen_cam"]] and r.cam_keep[:12].all()
    # a threshold just above and just below one kept track's worst error
    j = int(np.nonzero(keep)[0][5])
    for thresh, want in ((worst[j] * (1 + 1e-9), 1), (worst[j] * (1 - 1e-9), 0)):
        _, rr = solve("medium", 6, True, "pcg", float(thresh))
        assert rr.track_keep[j] == want
        np.testing.assert_array_equal(rr.point, r.point)  # the threshold does not reach the optimisation
    # no threshold: every participating track, no cheirality test
    _, rn = solve("medium", 6, True, "pcg", np.inf)
    assert rn.stats[8] == rn.stats[7] == 299 and rn.track_keep[e["behind_track"]]


def test_non_entries_are_copied_through_and_empty_problem_returns_early():
    s, r = solve("medium", 6, True)
    e = s["edge"]
    for c in (e["invalid_cam"], e["unseen_cam"]):
        assert np.array_equal(r.wRc[c], s["wRc"][c]) and np.array_equal(r.wtc[c], s["wtc"][c])
    assert np.array_equal(r.point[e["invalid_track"]], s["point"][e["invalid_track"]])
    assert r.stats[6] == 12 and r.stats[7] == 299
    s2 = dict(s, track_valid=np.zeros_like(s["track_valid"]))
    r2 = ref.global_ba_ref(*ref.call_args(s2))
    assert r2.stats.tolist() == [0.0] * 9 + [1.0] and not r2.track_keep.any() and not r2.cam_keep.any()
    assert np.array_equal(r2.wRc, s["wRc"]) and np.array_equal(r2.point, s["point"])


# ---------------------------------------------------------------- the host API, with the kernel call replaced
def _ba_data(s):
    from gtsfm_amd.bundle.bundle_adjustment import BaData
    from gtsfm_amd.common import geometry as g
    from gtsfm_amd.common.sfm_track import SfmTrack

    cams = {i: g.PinholeCameraCal3Bundler(g.Pose3(g.Rot3(s["wRc"][i]), s["wtc"][i]),
                                          g.Cal3Bundler(s["intr"][i, 0], 0, 0, s["intr"][i, 1], s["intr"][i, 2]))
            for i in range(len(s["intr"]))}
    tracks = []
    for j in range(len(s["offsets"]) - 1):
        t = SfmTrack(s["point"][j])
        for m in range(s["offsets"][j], s["offsets"][j + 1]):
            t.addMeasurement(int(s["img"][m]), s["uv"][m])
        tracks.append(t)
    return BaData(cams, tracks)


@pytest.fixture
def restated_kernel(monkeypatch):
    """device.global_ba answered by the restatement on CPU tensors, so that the host API runs without a GPU."""
    import torch

    from gtsfm_amd import device, native
    from gtsfm_amd.common import upload

    calls = []

    def fake(off, img, uv, point, tvalid, mvalid, wRc, wtc, intr, cvalid, **kw):
        calls.append(kw["reproj_error_thresh"])
        a = [None if x is None else x.numpy() for x in (off, img, uv, point, tvalid, mvalid, wRc, wtc, intr, cvalid)]
        r = ref.global_ba_ref(*a, robust=kw["robust"], measurement_sigma=kw["measurement_sigma"],
                              cam_pose3_prior_sigma=kw["cam_pose3_prior_sigma"], max_iterations=kw["max_iterations"],
                              pcg_rel_tol=kw["pcg_rel_tol"], pcg_max_iter=kw["pcg_max_iter"],
                              reproj_error_thresh=kw["reproj_error_thresh"])
        return device.GlobalBaResult(*(torch.from_numpy(np.ascontiguousarray(x)) for x in r[:6]))

    monkeypatch.setattr(device, "global_ba", fake)
    monkeypatch.setattr(native, "require_gpu", lambda: None)
    monkeypatch.setattr(upload, "cuda_device", lambda like=None: torch.device("cpu"))
    return calls


def test_run_ba_is_the_last_threshold_alone(restated_kernel):
    from gtsfm_amd.bundle.global_ba import GlobalBundleAdjustment

    data = _ba_data(ref.scene_small(1))
    opt3, fil3, mask3 = GlobalBundleAdjustment(reproj_error_thresholds=[10, 5, 3], robust_measurement_noise=True
                                               ).run_ba(data, [], {})
    assert restated_kernel == [3.0]  # one optimisation, the last threshold's filter
    opt1, fil1, mask1, err1 = GlobalBundleAdjustment(robust_measurement_noise=True).run_ba_stage_with_filtering(
        data, [], {}, 3)
    assert mask3 == mask1 and 0 < sum(mask1) < len(mask1) and err1 > 0
    assert len(fil3.tracks) == sum(mask1) == len(fil1.tracks) and sorted(fil3.cameras) == sorted(fil1.cameras)
    for a, b in zip(opt3.tracks, opt1.tracks):
        assert np.array_equal(a.point3(), b.point3()) and a.numberMeasurements() == b.numberMeasurements()
    for i in opt1.cameras:
        assert np.array_equal(opt3.cameras[i].pose().translation(), opt1.cameras[i].pose().translation())
    # no threshold: nothing is filtered
    _, fil, mask, _ = GlobalBundleAdjustment().run_ba_stage_with_filtering(data, [], {}, None)
    assert all(mask) and len(fil.tracks) == len(data.tracks)


def test_host_api_refusals_and_early_return(restated_kernel):
    from gtsfm_amd.bundle.bundle_adjustment import BaData, BundleAdjustmentOptimizer
    from gtsfm_amd.common import geometry as g

    data = _ba_data(ref.scene_small(1))
    ba = BundleAdjustmentOptimizer(reproj_error_thresholds=[3])
    with pytest.raises(NotImplementedError, match="relative-pose priors"):
        ba.run_ba(data, [], {(0, 1): object()})
    out = ba.run_ba_stage_with_filtering(BaData(data.cameras, []), [], {}, 3)
    assert out[0].tracks == [] and out[2] == [] and out[3] == 0.0 and restated_kernel == []
    out = ba.run_ba_stage_with_filtering(BaData({0: None}, data.tracks), [], {}, 3)
    assert out[2] == [False] * len(data.tracks) and out[3] == 0.0
    cams = dict(data.cameras)
    cams[0] = g.PinholeCameraCal3Bundler(cams[0].pose(), g.Cal3Bundler(1000, 0.1, 0, 500, 400))
    with pytest.raises(NotImplementedError, match="radial distortion"):
        ba.run_ba(BaData(cams, data.tracks), [], {})


def test_workspace_query_without_gpu():
    from gtsfm_amd import native

    q = native.lib().gtsfm_global_ba_workspace_bytes
    assert q(14000, 205000, 1000) > 205000 * 160
    assert q(40, 150, 5) > 0
    for shape in ((0, 150, 5), (40, 0, 5), (40, 150, 0), (-1, 150, 5), (2 ** 31, 150, 5), (40, 2 ** 31, 5),
                  (40, 150, 2 ** 20 + 1)):
        assert q(*shape) == 0
