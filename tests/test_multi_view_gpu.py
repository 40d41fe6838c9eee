"""gtsfm_assemble_ba_input, the device-camera path of data association and MultiViewOptimizer on the MI355X, against
the numpy restatement (tests/multi_view_ref.py).

Assemble: masks, lengths and statistics are integers and must equal the restatement's. Shapes: the six hand-written
cases; forty random draws of 64 cameras x 300 tracks of 1-6 measurements (more than one wavefront and more than one
workgroup of lanes); one chain of 4,096 cameras joined only by two-measurement tracks in a shuffled order next to a
chain of 4,095 (a deep union-find tree under contention, and a size comparison one apart).

The chain runs on one seeded scene (SCENE_SEED; build_scene): 10 cameras on a ring around 240 points, an island of 2
cameras with 40 points of their own and one two-view edge, and ring camera 4 whose keypoints are permuted in every
correspondence, so that each track through it fails triangulation. Relative poses are exact; keypoints are exact
projections rounded to float32. tests/multi_view_ref.chain_ref on this scene, run on the CPU before the seed was fixed,
drops exactly cameras 4, 10 and 11 (test_scene_conditions_hold_in_the_restatement repeats that check on every run).

Pose accuracy is measured against that restatement, not a number chosen in advance: its own largest camera-position
and rotation error against the scene's ground truth, after alignment (translation_averaging_ref.align_sim3 for the
positions, rotation_averaging_ref.aligned_angles_deg for the rotations), is the yardstick, and the GPU result must be
within ten times that, with a floor of 1e-6 of the scene extent and 1e-6 degrees. The factor covers the different LM and
PCG paths the per-stage tests already allow.
"""
import functools

import numpy as np
import pytest
import torch

from tests import multi_view_ref as M
from tests import rotation_averaging_ref, translation_averaging_ref, triangulation_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SCENE_SEED = 5
RING, ISLAND, BAD_CAM = 10, 2, 4
DROPPED = (BAD_CAM, RING, RING + 1)
TRI_THRESH = 3.0
FACTOR = 10.0


def _t(a, dtype=None):
    if a is None:
        return None
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))).to(DEV)


# ---------------------------------------------------------------- the assemble kernel
def _gpu_assemble(c, **kw):
    from gtsfm_amd import device

    r = device.assemble_ba_input(_t(c["offsets"], np.int32), _t(c["img"], np.int32), _t(c["track_valid"], np.uint8),
                                 _t(c["inlier"], np.uint8), _t(c["cam_valid"], np.uint8), c["n_img"],
                                 _t(c["extra_edges"], np.int32), **kw)
    return r


def _assert_equal(r, want, label):
    got = {k: getattr(r, k).cpu().numpy() for k in ("cam_keep", "track_keep", "track_len", "stats")}
    for k, v in got.items():
        np.testing.assert_array_equal(v, getattr(want, k), err_msg=f"{label}: {k}")


CASES = M.hand_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_assemble_hand_cases(name):
    case, cam_keep, track_keep, track_len, stats = CASES[name]
    r = _gpu_assemble(case)
    assert r.cam_keep.cpu().tolist() == cam_keep and r.track_keep.cpu().tolist() == track_keep
    assert r.track_len.cpu().tolist() == track_len and r.stats.cpu().tolist() == stats
    _assert_equal(r, M.run_case(case), name)


def test_assemble_random_draws():
    rng = np.random.default_rng(2024)
    n_components = []
    for k in range(40):
        case = M.random_case(rng, n_img=64, n_tracks=300)
        want = M.run_case(case)
        n_components.append(int(want.stats[0]))
        _assert_equal(_gpu_assemble(case), want, f"draw {k}")
    assert max(n_components) > 1  # the draws do exercise the selection


@functools.lru_cache(maxsize=None)
def _long_chains():
    """Cameras 0..4095 in one chain and 4096..8190 in another, each joined only by two-measurement tracks between
    neighbours of a random relabelling, all tracks in a shuffled order."""
    rng = np.random.default_rng(3)
    a, b = rng.permutation(4096), 4096 + rng.permutation(4095)
    tracks = [(int(a[i]), int(a[i + 1])) for i in range(4095)] + [(int(b[i]), int(b[i + 1])) for i in range(4094)]
    tracks = [list(tracks[i]) for i in rng.permutation(len(tracks))]
    return M.pack_case(tracks, 8191)


def test_assemble_long_chain():
    case = _long_chains()
    want = M.run_case(case)
    assert want.stats.tolist() == [2, 4096, 4095, 8190, 8189, 8191]
    assert want.cam_keep[:4096].all() and not want.cam_keep[4096:].any()
    _assert_equal(_gpu_assemble(case), want, "long chain")


def test_assemble_two_launches_byte_identical():
    case = _long_chains()
    r1, r2 = _gpu_assemble(case), _gpu_assemble(case)
    for k in ("cam_keep", "track_keep", "track_len", "stats"):
        assert getattr(r1, k).cpu().numpy().tobytes() == getattr(r2, k).cpu().numpy().tobytes(), k


def test_assemble_argument_checks():
    from gtsfm_amd import device, native

    L = native.lib()
    case = CASES["a_tie_first_track"][0]
    off, img = _t(case["offsets"], np.int32), _t(case["img"], np.int32)
    T, n_meas, n_img = 2, 6, 6
    need = L.gtsfm_assemble_ba_input_workspace_bytes(T, n_img)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    cam_keep = torch.empty(n_img, dtype=torch.uint8, device=DEV)
    track_keep = torch.empty(T, dtype=torch.uint8, device=DEV)
    track_len = torch.empty(T, dtype=torch.int32, device=DEV)
    stats = torch.full((6,), -1, dtype=torch.int64, device=DEV)

    def call(off_p=off.data_ptr(), n_tracks=T, nbytes=need, stats_p=stats.data_ptr()):
        return L.gtsfm_assemble_ba_input(off_p, img.data_ptr(), n_tracks, None, n_meas, None, None, None, n_img, None, 0,
                                         ws.data_ptr(), nbytes, cam_keep.data_ptr(), track_keep.data_ptr(),
                                         track_len.data_ptr(), stats_p, native.stream_handle())

    assert call() == native.GTSFM_OK
    assert call(off_p=None) == native.GTSFM_ERR_ARG
    assert call(stats_p=None) == native.GTSFM_ERR_ARG
    assert call(n_tracks=-1) == native.GTSFM_ERR_ARG
    assert call(nbytes=need - 1) == native.GTSFM_ERR_CAPACITY
    with pytest.raises(native.NativeError):
        _gpu_assemble(case, workspace_bytes=need - 1)
    assert call(n_tracks=0) == native.GTSFM_OK
    torch.cuda.synchronize()
    assert stats.cpu().tolist() == [0] * 6 and cam_keep.cpu().tolist() == [0] * n_img
    # a device track count below the capacity limits the tracks read: only the second triple is left of case (a)
    flipped = M.pack_case([[0, 1, 2], [3, 4, 5]], 6)
    n_dev = torch.tensor([1, 99], dtype=torch.int64, device=DEV)
    r = _gpu_assemble(flipped, n_tracks_dev=n_dev)
    _assert_equal(r, M.run_case(flipped, n_tracks=1), "n_tracks_dev")
    assert r.cam_keep.cpu().tolist() == [1, 1, 1, 0, 0, 0] and r.track_keep.cpu().tolist() == [1, 0]
    assert isinstance(device.BaInputResult, type)


def test_assemble_arrays_numpy_and_device():
    """DataAssociation.assemble_arrays over numpy and over device tensors, with extra edges."""
    from gtsfm_amd.data_association.data_assoc import DataAssociation, Tracks2d, Triangulated, assemble_metrics
    from gtsfm_amd.data_association.point3d_initializer import TriangulationOptions, TriangulationSamplingMode

    da = DataAssociation(2, TriangulationOptions(TriangulationSamplingMode.NO_RANSAC, TRI_THRESH))
    c = CASES["d_extra_edge"][0]
    want = M.run_case(c)
    T = len(c["offsets"]) - 1
    tracks = Tracks2d(c["offsets"], c["img"], None, None, None)
    tri = Triangulated(np.zeros(T, np.int32), None, None, c["inlier"], None)
    r = da.assemble_arrays(tracks, tri, c["track_valid"].astype(bool), c["cam_valid"], c["extra_edges"])
    assert isinstance(r.cam_keep, np.ndarray)
    for k in ("cam_keep", "track_keep", "track_len", "stats"):
        np.testing.assert_array_equal(getattr(r, k), getattr(want, k))
    tracks_d = Tracks2d(_t(c["offsets"]), _t(c["img"]), None, None, None)
    tri_d = Triangulated(_t(np.zeros(T, np.int32)), None, None, _t(c["inlier"]), None)
    rd = da.assemble_arrays(tracks_d, tri_d, _t(c["track_valid"]).bool(), _t(c["cam_valid"]), _t(c["extra_edges"]))
    assert rd.cam_keep.is_cuda
    _assert_equal(rd, want, "device")
    assert assemble_metrics(rd.stats, T) == {"accepted_tracks_ratio": 1.0, "num_accepted_tracks": 2,
                                             "number_cameras": 6}


# ---------------------------------------------------------------- device cameras through data association
def test_triangulation_camera_tuple_equals_camera_dict():
    from gtsfm_amd.common import geometry as g
    from gtsfm_amd.data_association.data_assoc import DataAssociation, Tracks2d
    from gtsfm_amd.data_association.point3d_initializer import TriangulationOptions, TriangulationSamplingMode

    off, img, uv, cams = triangulation_ref.load_door()
    n = len(cams.wRc)
    cam_dict = {i: g.PinholeCameraCal3Bundler(g.Pose3(g.Rot3(cams.wRc[i]), cams.wtc[i]),
                                              g.Cal3Bundler(cams.intr[i, 0], 0, 0, cams.intr[i, 1], cams.intr[i, 2]))
                for i in range(n) if i != 3}  # one camera missing: cam_valid 0 in the tuple
    valid = np.ones(n, np.uint8)
    valid[3] = 0
    wRc, wtc = cams.wRc.copy(), cams.wtc.copy()
    wRc[3], wtc[3] = np.eye(3), 0.0
    cam_tuple = (_t(wRc), _t(wtc), _t(cams.intr), _t(valid))
    tracks = Tracks2d(_t(off, np.int32), _t(img, np.int32), None, _t(uv), None)
    da = DataAssociation(3, TriangulationOptions(TriangulationSamplingMode.RANSAC_SAMPLE_UNIFORM, TRI_THRESH,
                                                 max_num_hypotheses=100))
    r1, v1 = da.run_triangulation_arrays(cam_dict, tracks)
    r2, v2 = da.run_triangulation_arrays(cam_tuple, tracks)
    for a, b in zip(tuple(r1) + (v1,), tuple(r2) + (v2,)):
        assert a.dtype == b.dtype and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert int(v1.sum()) > 1000


# ---------------------------------------------------------------- the chain
def build_scene(seed: int) -> dict:
    """See the module docstring. Arrays in the layout MultiViewOptimizer.run_arrays takes, plus the ground truth."""
    rng = np.random.default_rng(seed)
    n_img = RING + ISLAND
    ang = 2 * np.pi * np.arange(RING) / RING
    eyes = np.stack([10 * np.cos(ang), 10 * np.sin(ang), rng.uniform(-2.0, 2.0, RING)], 1)
    ring = triangulation_ref.lookat_cameras(eyes)
    centre = np.array([40.0, 0.0, 0.0])
    isl = triangulation_ref.lookat_cameras(np.array([[6.0, -2.0, 1.0], [6.0, 2.0, -1.0]]))
    wRc = np.concatenate([ring.wRc, isl.wRc])
    wtc = np.concatenate([ring.wtc, isl.wtc + centre])
    intr = np.concatenate([ring.intr, isl.intr])
    cams = triangulation_ref.Cameras(wRc, wtc, intr, np.ones(n_img, bool))
    pts = np.concatenate([rng.uniform(-2.0, 2.0, (240, 3)), centre + rng.uniform(-1.5, 1.5, (40, 3))])
    sees = np.zeros((n_img, len(pts)), bool)
    sees[:RING, :240] = rng.random((RING, 240)) < 0.6
    sees[RING:, 240:] = True
    coords, kp_of = [], np.full((n_img, len(pts)), -1)
    for i in range(n_img):
        p = np.flatnonzero(sees[i])
        uv, _ = triangulation_ref.project(cams, np.full(len(p), i), pts[p])
        coords.append(uv.astype(np.float32))
        kp_of[i, p] = np.arange(len(p))
    wrong = np.roll(np.arange(len(coords[BAD_CAM])), 7)  # the permuted keypoints of the corrupted camera
    pairs = [(i, j) for i in range(RING) for j in range(i + 1, RING)] + [(RING, RING + 1)]
    rows = []
    for i, j in pairs:
        both = np.flatnonzero(sees[i] & sees[j])
        ki, kj = kp_of[i, both], kp_of[j, both]
        ki = wrong[ki] if i == BAD_CAM else ki
        kj = wrong[kj] if j == BAD_CAM else kj
        rows.append(np.stack([ki, kj], 1).astype(np.int32))
    offsets = np.zeros(len(pairs) + 1, np.int32)
    np.cumsum([len(r) for r in rows], out=offsets[1:])
    pairs = np.array(pairs, np.int32)
    i1, i2 = pairs[:, 0], pairs[:, 1]
    i2Ri1 = np.einsum("nji,njk->nik", wRc[i2], wRc[i1])
    i2Ui1 = np.einsum("nji,nj->ni", wRc[i2], wtc[i1] - wtc[i2])
    i2Ui1 /= np.linalg.norm(i2Ui1, axis=1, keepdims=True)
    kp_count = np.array([len(c) for c in coords], np.int32)
    kmax = int(kp_count.max())
    kp_xy = np.zeros((n_img, kmax, 2), np.float32)
    for i, c in enumerate(coords):
        kp_xy[i, : len(c)] = c
    return dict(pairs=pairs, i2Ri1=i2Ri1, i2Ui1=i2Ui1, pair_valid=np.ones(len(pairs), np.uint8), offsets=offsets,
                v_corr=np.concatenate(rows), kp_count=kp_count, kmax=kmax, kp_xy=kp_xy, intrinsics=intr,
                num_images=n_img, gt=cams, coords=coords, rows=rows)


CHAIN_ARGS = ("pairs", "i2Ri1", "i2Ui1", "pair_valid", "offsets", "v_corr", "kp_count", "kmax", "kp_xy", "intrinsics",
              "num_images")


@functools.lru_cache(maxsize=None)
def _scene():
    return build_scene(SCENE_SEED)


@functools.lru_cache(maxsize=None)
def _chain_ref():
    s = _scene()
    return M.chain_ref(*(s[k] for k in CHAIN_ARGS), tri_thresh=TRI_THRESH, min_track_len=2)


def _modules():
    from gtsfm_amd.averaging.rotation.shonan import ShonanRotationAveraging
    from gtsfm_amd.averaging.translation.averaging_1dsfm import TranslationAveraging1DSFM
    from gtsfm_amd.bundle.bundle_adjustment import BundleAdjustmentOptimizer
    from gtsfm_amd.data_association.data_assoc import DataAssociation
    from gtsfm_amd.data_association.point3d_initializer import TriangulationOptions, TriangulationSamplingMode

    return (ShonanRotationAveraging(), TranslationAveraging1DSFM(),
            DataAssociation(2, TriangulationOptions(TriangulationSamplingMode.NO_RANSAC, TRI_THRESH)),
            BundleAdjustmentOptimizer())


def _optimizer():
    from gtsfm_amd.multi_view_optimizer import MultiViewOptimizer

    return MultiViewOptimizer(*_modules())


def _device_args():
    s = _scene()
    return [s[k] if k in ("kmax", "num_images") else _t(s[k]) for k in CHAIN_ARGS]


@functools.lru_cache(maxsize=None)
def _run_arrays():
    r = _optimizer().run_arrays(*_device_args())
    torch.cuda.synchronize()
    return r


def _pose_errors(wRc, wtc, cams_idx):
    """Largest position and rotation (degrees) error of the cameras cams_idx against the ground truth, after alignment."""
    gt = _scene()["gt"]
    pos = translation_averaging_ref.align_sim3(gt.wtc[cams_idx], np.asarray(wtc)[cams_idx])
    rot = rotation_averaging_ref.aligned_angles_deg(gt.wRc[cams_idx], np.asarray(wRc)[cams_idx])
    return float(np.linalg.norm(pos - gt.wtc[cams_idx], axis=1).max()), float(np.max(rot))


def _pose_bounds():
    ref = _chain_ref()
    kept = np.flatnonzero(ref.ba_in.cam_keep)
    e_pos, e_rot = _pose_errors(ref.ba.wRc, ref.ba.wtc, kept)
    extent = float(np.linalg.norm(_scene()["gt"].wtc[kept].max(0) - _scene()["gt"].wtc[kept].min(0)))
    return e_pos, e_rot, max(FACTOR * e_pos, 1e-6 * extent), max(FACTOR * e_rot, 1e-6)


def test_scene_conditions_hold_in_the_restatement():
    """CPU only in effect: the restatement alone drops exactly the island and the corrupted camera."""
    ref = _chain_ref()
    n = _scene()["num_images"]
    kept = sorted(set(range(n)) - set(DROPPED))
    assert np.flatnonzero(ref.rot.rot_valid).tolist() == list(range(RING))  # the island falls to rotation averaging
    assert ref.trans.wti_valid[BAD_CAM] == 1
    assert np.flatnonzero(ref.ba_in.cam_keep).tolist() == kept
    assert int(ref.ba.stats[6]) == len(kept) == 9 and int(ref.ba.stats[9]) == 0
    e_pos, e_rot, b_pos, b_rot = _pose_bounds()
    print(f"restatement against ground truth: position {e_pos:.3e}, rotation {e_rot:.3e} deg; "
          f"bounds {b_pos:.3e}, {b_rot:.3e} deg")


def _flatten(r):
    """Every tensor run_arrays returns, with a name."""
    out = [("keep", r.keep), ("valid", r.valid)]
    for name in ("rotations", "tracks", "translations", "triangulated", "ba_input", "ba"):
        stage = getattr(r, name)
        out += [(f"{name}.{f}", getattr(stage, f)) for f in stage._fields]
    out += [(f"cameras[{k}]", t) for k, t in enumerate(r.cameras)]
    return [(n, t) for n, t in out if t is not None]


def test_run_arrays_equals_the_stages_by_hand():
    from gtsfm_amd.data_association.dsf_tracks_estimator import DsfTracksEstimator
    from gtsfm_amd.multi_view_optimizer import MultiViewArrays, init_cameras_arrays

    got = _run_arrays()
    pairs, i2Ri1, i2Ui1, pair_valid, offsets, v_corr, kp_count, kmax, kp_xy, intr, n = _device_args()
    rot_m, trans_m, da, ba_m = _modules()
    keep = pair_valid  # no view-graph estimator: the island's edge reaches rotation averaging
    rot = rot_m.run_rotation_averaging_arrays(pairs, i2Ri1, keep, n)
    tracks = DsfTracksEstimator().run_arrays(pairs, offsets, v_corr, kp_count, kmax, valid=keep, kp_xy=kp_xy)
    trans = trans_m.run_translation_averaging_arrays(pairs, i2Ui1, rot.wRi, edge_valid=keep, rot_valid=rot.rot_valid,
                                                     track_offsets=tracks.offsets, track_img=tracks.image,
                                                     track_uv=tracks.uv, intrinsics=intr)
    cams = init_cameras_arrays(rot.wRi, trans.wti, trans.wti_valid, intr)
    tri, valid = da.run_triangulation_arrays(cams, tracks)
    ba_in = da.assemble_arrays(tracks, tri, valid, cams[3])
    ba = ba_m.run_ba_arrays((cams[0], cams[1], cams[2], ba_in.cam_keep), tracks, tri, ba_in.track_keep,
                            reproj_error_thresh=None)
    want = MultiViewArrays(keep, rot, tracks, trans, cams, tri, valid, ba_in, ba)
    a, b = _flatten(got), _flatten(want)
    assert [n for n, _ in a] == [n for n, _ in b]
    for (name, x), (_, y) in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape, name
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), name


def test_chain_drops_the_island_and_the_corrupted_camera():
    r = _run_arrays()
    s = _scene()
    n = s["num_images"]
    assert r.keep.cpu().tolist() == [1] * len(s["pairs"])  # the island's edge is in the view graph ...
    assert np.flatnonzero(r.rotations.rot_valid.cpu().numpy()).tolist() == list(range(RING))  # ... and pruned here
    assert r.translations.wti_valid.cpu().numpy()[list(range(RING))].all()
    assert int(r.translations.wti_valid[BAD_CAM]) == 1 and int(r.ba_input.cam_keep[BAD_CAM]) == 0
    kept = sorted(set(range(n)) - set(DROPPED))
    assert np.flatnonzero(r.ba_input.cam_keep.cpu().numpy()).tolist() == kept
    # no kept track holds a measurement of the corrupted camera
    img = r.tracks.image.cpu().numpy()
    track_of = np.repeat(np.arange(len(r.tracks.offsets) - 1), np.diff(r.tracks.offsets.cpu().numpy()))
    through_bad = np.unique(track_of[img == BAD_CAM])
    assert len(through_bad) > 0 and not r.ba_input.track_keep.cpu().numpy()[through_bad].any()
    stats = r.ba.stats.cpu().numpy()
    assert int(stats[6]) == 9 and int(stats[9]) == 0
    ref = _chain_ref()
    np.testing.assert_array_equal(r.ba_input.cam_keep.cpu().numpy(), ref.ba_in.cam_keep)


def test_chain_pose_accuracy_against_the_restatement():
    r = _run_arrays()
    kept = np.flatnonzero(_chain_ref().ba_in.cam_keep)
    e_pos, e_rot, b_pos, b_rot = _pose_bounds()
    g_pos, g_rot = _pose_errors(r.ba.wRc.cpu().numpy(), r.ba.wtc.cpu().numpy(), kept)
    print(f"run_arrays against ground truth: position {g_pos:.3e} (restatement {e_pos:.3e}, bound {b_pos:.3e}), "
          f"rotation {g_rot:.3e} deg (restatement {e_rot:.3e}, bound {b_rot:.3e})")
    assert g_pos <= b_pos and g_rot <= b_rot


def _dict_inputs():
    from gtsfm_amd.common import geometry as g
    from gtsfm_amd.common.keypoints import Keypoints

    s = _scene()
    keys = [tuple(int(v) for v in p) for p in s["pairs"]]
    return (s["num_images"], [Keypoints(c) for c in s["coords"]],
            {k: g.Rot3(R) for k, R in zip(keys, s["i2Ri1"])}, {k: g.Unit3(u) for k, u in zip(keys, s["i2Ui1"])},
            {k: rows for k, rows in zip(keys, s["rows"])},
            [g.Cal3Bundler(f, 0, 0, u0, v0) for f, u0, v0 in s["intrinsics"]])


def test_run_with_dicts():
    from gtsfm_amd.common import geometry as g

    ba_input, ba_output, ba_filtered = _optimizer().run(*_dict_inputs())
    r = _run_arrays()
    kept = np.flatnonzero(r.ba_input.cam_keep.cpu().numpy()).tolist()
    assert ba_input.get_valid_camera_indices() == kept == ba_output.get_valid_camera_indices()
    assert ba_input.number_tracks() == int(r.ba_input.stats[2]) == ba_output.number_tracks()
    assert ba_filtered.number_tracks() == int(r.ba.stats[8])
    assert all(t.numberMeasurements() >= 2 for t in ba_input.tracks)
    n = _scene()["num_images"]
    wRc, wtc = np.tile(np.eye(3), (n, 1, 1)), np.zeros((n, 3))
    for i, cam in ba_output.cameras.items():
        wRc[i], wtc[i] = g.camera_pose(cam)
    e_pos, e_rot, b_pos, b_rot = _pose_bounds()
    g_pos, g_rot = _pose_errors(wRc, wtc, np.array(kept))
    print(f"run against ground truth: position {g_pos:.3e} (bound {b_pos:.3e}), rotation {g_rot:.3e} deg (bound "
          f"{b_rot:.3e})")
    assert g_pos <= b_pos and g_rot <= b_rot


def test_run_degenerate_inputs_return_empty():
    num_images, keypoints, i2Ri1, i2Ui1, v_corr, intr = _dict_inputs()
    opt = _optimizer()
    for out in (opt.run(num_images, keypoints, {}, {}, {}, intr),
                opt.run(num_images, keypoints, {k: None for k in i2Ri1}, {k: None for k in i2Ui1}, v_corr, intr)):
        assert len(out) == 3
        for data in out:
            assert data.cameras == {} and data.tracks == []
    with pytest.raises(NotImplementedError):
        opt.run(num_images, keypoints, i2Ri1, i2Ui1, v_corr, intr, relative_pose_priors={(0, 1): object()})
