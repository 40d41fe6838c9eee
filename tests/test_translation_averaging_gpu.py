"""GPU: holds the gtsfm_transavg_* kernels (gtsfm_amd/csrc/transavg.hip) to the numpy restatement
(tests/translation_averaging_ref.py): measurements and track selection exactly (directions within 4 ulp), MFAS exactly
(violated sets, bit-equal outlier sums), the recovery in its decisions and, in the shared gauge, in its positions."""
import numpy as np
import pytest
import torch

from tests import tracks_ref
from tests import translation_averaging_ref as ref
from tests import translation_averaging_scenes as scenes

pytestmark = pytest.mark.gpu

# 40 cameras, about half of the pairs as edges, 10 % of them planted outliers. The recovery test uses it without tracks
# (11 LM iterations, smallest decision margin of the restatement 9.8e-6): with this scene's tracks a landmark is left
# nearly free along its rays and the restatement differs from itself by 4e-4 of the extent when its measurements are
# reordered, so positions say nothing there. The door scene covers the recovery with tracks.
SCENE40_SEED = 5
NEAR_TIE_DIRECTIONS = 0  # of the 64 directions of scenes.mfas_graph(); tests/test_translation_averaging.py checks it
POSITION_CEILING = 1e-6  # relative to the scene's extent


def _dev():
    return torch.device("cuda:0")


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _measure(case, edge_valid=None, rot_valid=None):
    from gtsfm_amd import device

    has = "offsets" in case
    return device.transavg_measurements(_t(case["edges"]), _t(case["i2Ui1"]), _t(edge_valid), _t(case["wRi"]),
                                        _t(rot_valid), _t(case["offsets"]) if has else None,
                                        _t(case["img"]) if has else None, _t(case["uv"]) if has else None,
                                        _t(case["intr"]) if has else None)


def _scene40():
    return ref.seeded_scene(40, SCENE40_SEED)


def _scene40_tracks():
    return ref.seeded_scene(40, SCENE40_SEED, n_pts=200)


CASES = {"circle": lambda: scenes.sample_case("circle_all_edges"), "panorama": lambda: scenes.sample_case("panorama"),
         "door": lambda: scenes.door(False), "door_tracks": lambda: scenes.door(True), "scene40": _scene40}


def _ulp_diff(a, b):
    return np.abs(a - b) / np.maximum(np.spacing(np.maximum(np.abs(a), np.abs(b))), np.finfo(np.float64).tiny)


@pytest.mark.parametrize("name", ["door_tracks", "scene40"])
def test_measurements_and_selection(name):
    case = CASES[name]() if name != "scene40" else _scene40_tracks()
    n_img = len(case["wRi"])
    ev = np.ones(len(case["edges"]), np.uint8)
    rv = np.ones(n_img, np.uint8)
    if name == "scene40":
        ev[4] = 0
        rv[0] = 0  # camera 0 stays valid as the i1 of its edges: its track measurements are counted, not written
    got = _measure(case, ev, rv)
    want = ref.measurements(case["edges"], case["i2Ui1"], ev, case["wRi"], rv, case["offsets"], case["img"], case["uv"],
                            case["intr"])
    counts = got.counts.cpu().numpy()
    print(name, "counts", counts.tolist(), "selected", len(want.selected))
    np.testing.assert_array_equal(counts, want.counts)
    ns = int(counts[2])
    assert ns > 0
    np.testing.assert_array_equal(got.selected.cpu().numpy()[:ns], want.selected)
    assert (got.selected.cpu().numpy()[ns:] == -1).all()
    np.testing.assert_array_equal(got.cam_valid.cpu().numpy(), want.cam_valid)
    np.testing.assert_array_equal(got.key.cpu().numpy(), want.key)
    np.testing.assert_array_equal(got.valid.cpu().numpy(), want.valid)
    ulp = _ulp_diff(got.dir.cpu().numpy(), want.dir)
    print(name, "direction difference, ulp:", ulp.max())
    assert ulp.max() <= 4


def test_select_tracks_reference_table():
    g = scenes.golden("select_tracks")
    tc = g["track_cameras"]
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in tc])]).astype(np.int32)
    img = np.concatenate(tc).astype(np.int32)
    edges = np.array([(0, 1), (1, 2), (2, 3)], np.int32)  # valid cameras 0..3
    case = dict(edges=edges, i2Ui1=np.tile([1.0, 0, 0], (3, 1)), wRi=np.tile(np.eye(3), (7, 1, 1)), offsets=offsets,
                img=img, uv=np.full((len(img), 2), 20.0), intr=np.tile([20.0, 0.0, 0.0], (7, 1)))
    from gtsfm_amd import device

    got = device.transavg_measurements(_t(edges), _t(case["i2Ui1"]), None, _t(case["wRi"]), None, _t(offsets), _t(img),
                                       _t(case["uv"]), _t(case["intr"]), measurements_per_camera=3)
    want, _ = ref.select_tracks(offsets, img, [1, 1, 1, 1, 0, 0, 0], 3)
    assert got.counts.cpu().numpy()[2] == 4
    np.testing.assert_array_equal(got.selected.cpu().numpy()[:4], want)
    d = got.dir.cpu().numpy()[3]
    np.testing.assert_allclose(d, np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0), rtol=0, atol=2e-16)


def test_mfas_graph_matches_sequential_restatement():
    from gtsfm_amd import device

    g = scenes.mfas_graph()
    want = ref.mfas(g["key"], g["dir"], g["valid"], g["n_nodes"], g["proj"])
    near = want.margins < ref.NEAR_TIE
    assert int(near.sum()) == NEAR_TIE_DIRECTIONS and near.mean() <= 0.01
    osum, inlier, viol = device.transavg_mfas(_t(g["key"]), _t(g["dir"]), _t(g["valid"]), g["n_nodes"], _t(g["proj"]),
                                              want_violated=True)
    mask = ref.violated_bits_to_mask(viol.cpu().numpy().view(np.uint32), len(g["key"]))
    for di in np.nonzero(~near)[0]:
        assert np.array_equal(mask[di], want.violated[di]), f"direction {di}: violated sets differ"
    print("violated per direction:", want.violated.sum(1).min(), "-", want.violated.sum(1).max(), "inliers",
          int(want.inlier.sum()), "of", len(want.inlier))
    assert np.array_equal(osum.cpu().numpy().view(np.uint64), want.outlier_sum.view(np.uint64))
    np.testing.assert_array_equal(inlier.cpu().numpy(), want.inlier)


def test_mfas_small_graphs():
    from gtsfm_amd import device

    c = scenes.sample_case("all_outliers")
    ms = ref.measurements(c["edges"], c["i2Ui1"], None, c["wRi"], None)
    proj = ref.sample_uniform_directions(scenes.N_DIR, scenes.SEED)
    want = ref.mfas(ms.key, ms.dir, ms.valid, 5, proj)
    osum, inlier, _ = device.transavg_mfas(_t(ms.key), _t(ms.dir), _t(ms.valid), 5, _t(proj))
    assert np.array_equal(osum.cpu().numpy().view(np.uint64), want.outlier_sum.view(np.uint64))
    np.testing.assert_array_equal(inlier.cpu().numpy(), want.inlier)
    assert not inlier.cpu().numpy()[[3, 6, 8, 9]].any()  # every edge of camera 4
    key, d = np.array([[1, 0]], np.int32), np.array([[0.0, 0.6, 0.8]])
    want = ref.mfas(key, d, None, 2, proj[:8])
    osum, inlier, viol = device.transavg_mfas(_t(key), _t(d), None, 2, _t(proj[:8]), want_violated=True)
    assert osum.item() == 0.0 and inlier.item() == 1 and not viol.cpu().numpy().any() and not want.violated.any()


@pytest.fixture(scope="module")
def rounding_floor():
    """The restatement against itself on the door scene with the measurements after the first reversed, relative to the
    scene's extent (tests/test_translation_averaging.py prints the same figure)."""
    case = scenes.door(True)
    ms, mf, rec = ref.run_1dsfm(case["edges"], case["i2Ui1"], case["wRi"], None, case["offsets"], case["img"],
                                case["uv"], case["intr"], n_dir=scenes.N_DIR, seed=scenes.SEED)
    n = len(case["edges"]) + int(ms.counts[1])
    order = np.concatenate([[0], np.arange(n - 1, 0, -1)])
    rev = ref.recover(ms.key[:n][order], ms.dir[:n][order], mf.inlier[order], 12, len(ms.selected), None, True, 1.0,
                      scenes.SEED)
    extent = np.linalg.norm(rec.wti - rec.wti.mean(0), axis=1).max()
    return max(np.abs(rev.wti - rec.wti).max(), np.abs(rev.landmark - rec.landmark).max()) / extent


@pytest.mark.parametrize("name", list(CASES))
def test_recovery_matches_restatement(name, rounding_floor):
    from gtsfm_amd import device

    case = CASES[name]()
    n_img = len(case["wRi"])
    ms = _measure(case)
    counts = ms.counts.cpu().numpy()
    n, n_land = len(case["edges"]) + int(counts[1]), int(counts[2])
    key, d, valid = ms.key[:n].contiguous(), ms.dir[:n].contiguous(), ms.valid[:n].contiguous()
    proj = ref.sample_uniform_directions(scenes.N_DIR, scenes.SEED)
    _, inlier, _ = device.transavg_mfas(key, d, valid, n_img + n_land, _t(proj))
    got = device.transavg_recover(key, d, inlier, n_img, n_land, None, True, 1.0, scenes.SEED)
    want = ref.recover(key.cpu().numpy(), d.cpu().numpy(), inlier.cpu().numpy(), n_img, n_land, None, True, 1.0,
                       scenes.SEED)
    gs = got.stats.cpu().numpy()
    print(name, "gpu stats", gs.tolist(), "restatement", want.stats.tolist(), "min LM margin", want.min_margin)
    assert want.min_margin > 1e-6, "pick another seed: an LM decision of the restatement is within 1e-6 of its threshold"
    for k in (2, 3, 5, 6, 7, 8, 9):  # LM iterations, trials, cap hits, sets, factors, valid cameras, status
        assert gs[k] == want.stats[k], (k, gs[k], want.stats[k])
    assert abs(gs[4] - want.stats[4]) <= 2 * max(want.stats[3], 1)
    np.testing.assert_array_equal(got.wti_valid.cpu().numpy(), want.wti_valid)
    np.testing.assert_array_equal(got.landmark_valid.cpu().numpy(), want.landmark_valid)
    extent = max(np.linalg.norm(want.wti - want.wti.mean(0), axis=1).max(), 1e-300) if name != "panorama" else 1.0
    diff = np.abs(got.wti.cpu().numpy() - want.wti).max() / extent
    if n_land:
        diff = max(diff, np.abs(got.landmark.cpu().numpy() - want.landmark).max() / extent)
    tol = min(10.0 * rounding_floor, POSITION_CEILING)
    print(name, "position difference / extent", diff, "floor", rounding_floor, "tolerance", tol)
    np.testing.assert_allclose(gs[:2], want.stats[:2], rtol=1e-9, atol=1e-18)
    assert diff <= tol
    if name == "scene40":
        aligned = ref.align_sim3(case["wti"], got.wti.cpu().numpy())
        assert np.abs(aligned - case["wti"]).max() < 0.1  # planted outliers rejected: the ring is recovered


def test_two_launches_are_byte_identical():
    from gtsfm_amd import device

    case = scenes.door(True)
    a, b = _measure(case), _measure(case)
    for f in ("key", "dir", "valid", "selected", "cam_valid", "counts"):
        assert torch.equal(getattr(a, f).view(torch.uint8), getattr(b, f).view(torch.uint8)), f
    n = len(case["edges"]) + int(a.counts[1].item())
    n_land = int(a.counts[2].item())
    key, d, valid = a.key[:n].contiguous(), a.dir[:n].contiguous(), a.valid[:n].contiguous()
    proj = _t(ref.sample_uniform_directions(256, 1))
    m1 = device.transavg_mfas(key, d, valid, 12 + n_land, proj, want_violated=True)
    m2 = device.transavg_mfas(key, d, valid, 12 + n_land, proj, want_violated=True)
    for x, y in zip(m1, m2):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    r1 = device.transavg_recover(key, d, m1[1], 12, n_land, seed=5)
    r2 = device.transavg_recover(key, d, m1[1], 12, n_land, seed=5)
    for f in ("wti", "wti_valid", "landmark", "landmark_valid", "stats"):
        assert torch.equal(getattr(r1, f).view(torch.uint8), getattr(r2, f).view(torch.uint8)), f


def test_class_and_array_routes_agree():
    from gtsfm_amd.averaging.translation import TranslationAveraging1DSFM
    from gtsfm_amd.common import geometry
    from gtsfm_amd.common.sfm_track import SfmMeasurement, SfmTrack2d

    case = scenes.door(True)
    # Unit3 renormalises (and not idempotently): both routes get the numbers held by the same Unit3 objects
    units = [geometry.Unit3(u) for u in case["i2Ui1"]]
    case["i2Ui1"] = np.array([geometry.unit_vector(U) for U in units])
    obj = TranslationAveraging1DSFM()
    arr = obj.run_translation_averaging_arrays(_t(case["edges"]), _t(case["i2Ui1"]), _t(case["wRi"]),
                                               track_offsets=_t(case["offsets"]), track_img=_t(case["img"]),
                                               track_uv=_t(case["uv"]), intrinsics=_t(case["intr"]))
    assert arr.wti.is_cuda and arr.wti.dtype == torch.float64 and arr.wti_valid.dtype == torch.uint8
    off, img, uv = case["offsets"], case["img"], case["uv"]
    tracks = [SfmTrack2d([SfmMeasurement(int(img[m]), uv[m].astype(np.float64)) for m in range(off[t], off[t + 1])])
              for t in range(len(off) - 1)]
    f, u0, v0 = (float(x) for x in case["intr"][0])
    cals = [geometry.Cal3Bundler(f, 0.0, 0.0, u0, v0)] * 12
    i2Ui1 = {(int(a), int(b)): U for (a, b), U in zip(case["edges"], units)}
    poses, metrics = obj.run_translation_averaging(12, i2Ui1, [geometry.Rot3(R) for R in case["wRi"]], tracks, cals)
    assert metrics["num_total_1dsfm_measurements"] == 66 and metrics["num_translations_estimated"] == 12
    assert metrics["num_inlier_1dsfm_measurements"] + metrics["num_outlier_1dsfm_measurements"] == 66
    wti = arr.wti.cpu().numpy()
    for i, p in enumerate(poses):
        assert np.array_equal(np.asarray(p.translation()), wti[i])

    c = scenes.sample_case("all_outliers")
    poses, metrics = obj.run_translation_averaging(5, {(int(a), int(b)): u for (a, b), u in zip(c["edges"], c["i2Ui1"])},
                                                   list(c["wRi"]))
    assert len(poses) == 5 and poses[-1] is None and all(p is not None for p in poses[:4])
    assert metrics["num_translations_estimated"] == 4
    poses, _ = obj.run_translation_averaging(3, {(0, 1): np.array([0.0, 0.0, 1.0]), (0, 2): None}, [np.eye(3)] * 3)
    assert poses[2] is None and poses[0] is not None and poses[1] is not None


def test_chain_tracks_to_translations_to_triangulation():
    from gtsfm_amd import device, native
    from gtsfm_amd.averaging.translation import TranslationAveraging1DSFM

    scene = tracks_ref.make_scene(8, 64, n_points=120, vis_prob=0.6, seed=2)
    t_off, t_img, t_kp, t_uv, stats = device.tracks_from_matches(_t(scene.pairs), _t(scene.offsets), _t(scene.v_corr),
                                                                 _t(scene.kp_count), scene.kmax, valid=_t(scene.valid),
                                                                 kp_xy=_t(scene.kp_xy))
    rng = np.random.default_rng(0)
    u = rng.normal(size=(len(scene.pairs), 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    wRi = _t(np.tile(np.eye(3), (8, 1, 1)))
    intr = _t(np.tile(np.array([500.0, 320.0, 240.0]), (8, 1)))
    res = TranslationAveraging1DSFM().run_translation_averaging_arrays(
        _t(np.asarray(scene.pairs, np.int32)), _t(u), wRi, track_offsets=t_off, track_img=t_img, track_uv=t_uv,
        intrinsics=intr, n_tracks_dev=stats)
    for x, dt in ((res.wti, torch.float64), (res.wti_valid, torch.uint8), (res.landmark, torch.float64),
                  (res.selected, torch.int32), (res.inlier, torch.uint8), (res.stats, torch.float64)):
        assert x.is_cuda and x.dtype == dt
    tri = device.triangulate_tracks(t_off, t_img, t_uv, wRi, res.wti, intr, res.wti_valid, native.GTSFM_TRI_NO_RANSAC,
                                    3.0, n_tracks_dev=stats)
    assert tri.point.is_cuda and tri.point.dtype == torch.float64 and tri.exit_code.dtype == torch.int32
