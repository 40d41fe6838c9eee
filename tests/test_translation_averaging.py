"""CPU: pins the numpy restatement of 1DSfM translation averaging (tests/translation_averaging_ref.py) to the
reference's own test cases (tests/averaging/translation/test_averaging_1dsfm.py), whose data lives under
tests/golden/translation_averaging/, and checks the Python surface that needs no GPU."""
import pickle

import numpy as np
import pytest

from tests import translation_averaging_ref as ref
from tests import translation_averaging_scenes as scenes

RELATIVE_ERROR_THRESHOLD = 3e-2  # the reference test's compare_global_poses arguments
ABSOLUTE_ERROR_THRESHOLD = 3e-1


def _run(case, **kw):
    return ref.run_1dsfm(case["edges"], case["i2Ui1"], case["wRi"], None, case.get("offsets"), case.get("img"),
                         case.get("uv"), case.get("intr"), n_dir=scenes.N_DIR, seed=scenes.SEED, **kw)


@pytest.fixture(scope="module")
def solved():
    cases = {"circle": scenes.sample_case("circle_all_edges"), "panorama": scenes.sample_case("panorama"),
             "door": scenes.door(False), "door_tracks": scenes.door(True)}
    return {k: (c, _run(c)) for k, c in cases.items()}


def test_select_tracks_reference_table():
    g = scenes.golden("select_tracks")
    tc = g["track_cameras"]
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in tc])])
    cam_valid = np.zeros(7, np.uint8)
    cam_valid[g["valid_cameras"]] = 1
    selected, cams = ref.select_tracks(offsets, np.concatenate(tc), cam_valid, g["measurements_per_camera"])
    assert len(selected) == g["num_expected"] == 4
    for t in selected:
        assert cams[t] in g["expected_track_cameras"]
    assert selected[0] == 0  # the longest track first (np.argmax takes the first maximum)


def test_landmark_direction_exact():
    ms = ref.measurements([[0, 1]], [[1.0, 0.0, 0.0]], None, np.array([np.diag([1.0, -1.0, 1.0])] * 2), None,
                          [0, 3], [0, 1, 0], [[20.0, 20.0]] * 3, [[20.0, 0.0, 0.0]] * 2, per_cam=3)
    assert ms.selected == [0] and ms.counts[1] == 3
    expected = np.array([1.0, -1.0, 1.0]) / np.linalg.norm([1.0, -1.0, 1.0])
    assert np.array_equal(ms.dir[1], expected)
    assert tuple(ms.key[1]) == (0, 2)


@pytest.mark.parametrize("name", ["circle", "panorama", "door", "door_tracks"])
def test_pose_cases_meet_reference_thresholds(solved, name):
    case, (ms, mf, rec) = solved[name]
    assert rec.stats[9] == 0 and rec.wti_valid.all()
    aligned = ref.align_sim3(case["wti"], rec.wti)
    err = np.abs(aligned - case["wti"])
    print(name, "max aligned error", err.max(), "LM", rec.stats[2:6], "selected tracks", len(ms.selected))
    # compare_global_poses(computed, expected, 3e-2, 3e-1): rotations (the inputs) within 3e-2 degrees, translations
    # np.allclose(atol 3e-1, rtol 1e-1); the tighter reading, 3e-2 relative to the scene's extent, holds as well
    assert np.allclose(aligned, case["wti"], atol=ABSOLUTE_ERROR_THRESHOLD, rtol=1e-1)
    extent = max(np.linalg.norm(case["wti"] - case["wti"].mean(0), axis=1).max(), 1.0)
    assert err.max() <= RELATIVE_ERROR_THRESHOLD * extent
    if name == "door_tracks":
        assert len(ms.selected) > 0 and rec.landmark_valid.sum() > 0


def test_all_outliers_returns_none_for_last_camera():
    c = scenes.sample_case("all_outliers")
    ms, mf, rec = _run(c)
    assert len(rec.wti_valid) == 5
    assert rec.wti_valid.tolist() == [1, 1, 1, 1, 0]
    assert mf.margins.min() > ref.NEAR_TIE


def test_pcg_matches_exact_solve(solved):
    case, (ms, mf, rec) = solved["door_tracks"]
    n = len(case["edges"]) + int(ms.counts[1])
    ex = ref.recover(ms.key[:n], ms.dir[:n], mf.inlier, 12, len(ms.selected), None, True, 1.0, scenes.SEED,
                     pcg_rel_tol=1e-10, solver="exact")
    print("pcg vs exact: max |dt|", np.abs(ex.wti - rec.wti).max(), "landmarks", np.abs(ex.landmark - rec.landmark).max())
    assert ex.stats[2] == rec.stats[2] and ex.stats[3] == rec.stats[3]
    assert np.abs(ex.wti - rec.wti).max() < 1e-6


def test_restatement_rounding_floor(solved):
    """The floor the GPU test scales its tolerance from: the door scene again with the measurements after the first
    (which carries the gauge and the scale) in reverse order."""
    case, (ms, mf, rec) = solved["door_tracks"]
    n = len(case["edges"]) + int(ms.counts[1])
    order = np.concatenate([[0], np.arange(n - 1, 0, -1)])
    rev = ref.recover(ms.key[:n][order], ms.dir[:n][order], mf.inlier[order], 12, len(ms.selected), None, True, 1.0,
                      scenes.SEED)
    assert mf.inlier[0] == 1
    extent = np.linalg.norm(rec.wti - rec.wti.mean(0), axis=1).max()
    floor = max(np.abs(rev.wti - rec.wti).max(), np.abs(rev.landmark - rec.landmark).max()) / extent
    print("rounding floor relative to the extent:", floor)
    assert rev.stats[2] == rec.stats[2] and rev.stats[3] == rec.stats[3]
    assert floor < 1e-7


def test_mfas_graph_has_no_near_tie():
    g = scenes.mfas_graph()
    assert len(g["key"]) == 1515 and len(g["key"]) % 64 != 0
    r = ref.mfas(g["key"], g["dir"], g["valid"], g["n_nodes"], g["proj"])
    assert int((r.margins < ref.NEAR_TIE).sum()) == 0
    deg = np.bincount(g["key"][g["valid"] == 1].ravel(), minlength=g["n_nodes"])
    assert deg[g["isolated"]] == 0 and deg[g["sink"]] == 5
    assert r.violated.any() and 0 < r.inlier.sum() < len(r.inlier)  # cycles exist: the heuristic branch ran


def test_class_surface():
    from gtsfm_amd.averaging.translation import TranslationAveraging1DSFM, TranslationAveragingBase

    obj = TranslationAveraging1DSFM()
    assert isinstance(obj, TranslationAveragingBase)
    clone = pickle.loads(pickle.dumps(obj))
    assert type(clone) is type(obj) and clone._seed == obj._seed == scenes.SEED
    d = obj.sample_projection_directions(None)
    assert d.shape == (2000, 3) and np.array_equal(d, ref.sample_uniform_directions(2000, scenes.SEED))
    kde = TranslationAveraging1DSFM(projection_sampling_method="SAMPLE_WITH_INPUT_DENSITY")
    with pytest.raises(NotImplementedError):
        kde.run_translation_averaging(2, {(0, 1): np.array([1.0, 0, 0])}, [np.eye(3)] * 2)
    with pytest.raises(NotImplementedError):
        obj.run_translation_averaging(2, {(0, 1): np.array([1.0, 0, 0])}, [np.eye(3)] * 2, i2Ti1_priors={(0, 1): object()})
    with pytest.raises(NotImplementedError):
        obj.run_translation_averaging(2, {(0, 1): np.array([1.0, 0, 0])}, [np.eye(3)] * 2, absolute_pose_priors=[object()])


def test_abi_is_407():
    from gtsfm_amd import native

    assert native.ABI_VERSION == 407 and native.lib().gtsfm_hip_abi_version() == 407
    for name in ("gtsfm_transavg_measurements", "gtsfm_transavg_mfas", "gtsfm_transavg_recover"):
        assert name in native.SIGNATURES
    L = native.lib()
    assert L.gtsfm_transavg_mfas_workspace_bytes(1000, native.TA_MFAS_MAX_NODES, 64) > 0
    assert L.gtsfm_transavg_mfas_workspace_bytes(1000, native.TA_MFAS_MAX_NODES + 1, 64) == 0
