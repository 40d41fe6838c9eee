"""gtsfm_tracks_from_matches on the MI355X against tests/tracks_ref.py (the reference route in numpy / scipy).

Everything is integer work or a gather, so every comparison is exact: the five stats, offsets / image / keypoint as
arrays, uv bitwise. Shapes are the smallest that still reach every path: row counts around the 256-lane workgroup,
more rows than one pass of the union kernel's grid (2,048 workgroups x 256 rows; `scene300` has more), node counts
past one 2,048-node scan tile, parent chains longer than a wave and than a workgroup (`chain`), thousands of lanes
hooking onto one root (`giant_invalid`).
"""
import functools

import numpy as np
import pytest
import torch

import tracks_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _gpu(scene, kp_xy=True, track_cap=None, meas_cap=None, out=None):
    """The raw launch: full-capacity device outputs and the stats, as numpy."""
    from gtsfm_amd import device

    dev = torch.device(DEV)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    res = device.tracks_from_matches(t(scene.pairs), t(scene.offsets), t(scene.v_corr), t(scene.kp_count), scene.kmax,
                                     valid=t(scene.valid), kp_xy=t(scene.kp_xy) if kp_xy else None,
                                     track_cap=track_cap, meas_cap=meas_cap, out=out)
    return tuple(None if a is None else a.cpu().numpy() for a in res)


def _compare(got, want, label):
    t_off, t_img, t_kp, t_uv, stats = got
    print(f"{label}: stats {stats.tolist()} (reference {want.stats.tolist()})")
    np.testing.assert_array_equal(stats, want.stats, err_msg=label)
    n_tracks, n_meas = int(stats[0]), int(stats[1])
    np.testing.assert_array_equal(t_off[: n_tracks + 1], want.offsets, err_msg=label)
    np.testing.assert_array_equal(t_img[:n_meas], want.image, err_msg=label)
    np.testing.assert_array_equal(t_kp[:n_meas], want.keypoint, err_msg=label)
    if want.uv is not None and t_uv is not None:
        assert t_uv[:n_meas].tobytes() == want.uv.tobytes(), f"{label}: uv is not the gathered kp_xy"


def _reference(scene):
    return ref.reference_tracks(scene.pairs, scene.offsets, scene.v_corr, scene.kp_count, scene.kmax, scene.valid,
                                scene.kp_xy)


def _scene_of_rows(pairs, rows_per_pair, n_img, kmax, valid=None, kp_count=None, seed=0):
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    rows = [np.asarray(r, np.int32).reshape(-1, 2) for r in rows_per_pair]
    offsets = np.zeros(len(rows) + 1, np.int32)
    np.cumsum([len(r) for r in rows], out=offsets[1:])
    v_corr = np.concatenate(rows) if rows else np.zeros((0, 2), np.int32)
    kp_count = np.full(n_img, kmax, np.int32) if kp_count is None else np.asarray(kp_count, np.int32)
    kp_xy = np.random.default_rng(seed).random((n_img, kmax, 2), dtype=np.float32)
    return ref.Scene(pairs, offsets, v_corr, kp_count, kmax, None if valid is None else np.asarray(valid, np.uint8),
                     kp_xy)


@functools.lru_cache(maxsize=None)
def _scene300():
    """(scene, its reference result): generated and evaluated once, shared, never modified."""
    scene = ref.make_scene(300, 512, n_points=9000, vis_prob=0.12, vis_spread=0.95, match_prob=0.45, wrong_share=0.03,
                           seed=0)
    return scene, _reference(scene)


# ---- golden cases ----

@pytest.mark.parametrize("name", ref.GOLDEN_CASES)
def test_golden_run(name):
    from gtsfm_amd.common.keypoints import Keypoints
    from gtsfm_amd.data_association.dsf_tracks_estimator import CppDsfTracksEstimator, DsfTracksEstimator, get_2d_tracks

    matches, coords, case = ref.load_golden(name)
    kps = [Keypoints(c) for c in coords]
    tracks = DsfTracksEstimator().run(matches, kps)
    assert len(tracks) == case["n_tracks"]
    assert all(t.validate_unique_cameras() for t in tracks)
    assert CppDsfTracksEstimator is DsfTracksEstimator
    assert get_2d_tracks(matches, kps) == tracks
    want = ref.reference_tracks_from_dict(matches, coords)
    for t, track in enumerate(tracks):
        lo, hi = want.offsets[t], want.offsets[t + 1]
        assert [m.i for m in track.measurements] == want.image[lo:hi].tolist()
        for m, i, k in zip(track.measurements, want.image[lo:hi], want.keypoint[lo:hi]):
            np.testing.assert_array_equal(m.uv, coords[i][k])


@pytest.mark.parametrize("name", ref.GOLDEN_CASES)
@pytest.mark.parametrize("kind", ["numpy", "torch_cpu", "torch_gpu"])
def test_golden_run_arrays(name, kind):
    from gtsfm_amd.data_association.dsf_tracks_estimator import DsfTracksEstimator, Tracks2d

    matches, coords, case = ref.load_golden(name)
    kp_count, kmax, kp_xy = ref.pack_keypoints(coords)
    args = list(ref.csr_from_dict(matches)) + [kp_count]
    if kind != "numpy":
        dev = torch.device(DEV if kind == "torch_gpu" else "cpu")
        args = [torch.from_numpy(a).to(dev) for a in args]
        xy = torch.from_numpy(kp_xy).to(dev)
    else:
        xy = kp_xy
    got = DsfTracksEstimator().run_arrays(*args, kmax, kp_xy=xy)
    assert isinstance(got, Tracks2d)
    for a in got:
        if kind == "numpy":
            assert isinstance(a, np.ndarray)
        else:
            assert isinstance(a, torch.Tensor) and a.device == args[0].device
    got = [np.asarray(a.cpu()) if kind != "numpy" else a for a in got]
    want = ref.reference_tracks_from_dict(matches, coords)
    assert int(got[4][0]) == case["n_tracks"]
    _compare(got, want, f"{name}/{kind}")
    assert len(got[0]) == want.stats[0] + 1 and len(got[1]) == want.stats[1] and len(got[3]) == want.stats[1]


def test_three_images_index_wise():
    """test_dsf_tracks_estimator.py:86-112: the three tracks, measurement by measurement, in canonical order."""
    from gtsfm_amd.common.keypoints import Keypoints
    from gtsfm_amd.data_association.dsf_tracks_estimator import DsfTracksEstimator

    matches, coords, case = ref.load_golden("three_images")
    tracks = DsfTracksEstimator().run(matches, [Keypoints(c) for c in coords])
    assert len(tracks) == 3
    for track, want in zip(tracks, case["tracks"]):
        assert track.number_measurements() == len(want)
        for j, w in enumerate(want):
            assert track.measurement(j).i == w["i"]
            np.testing.assert_array_equal(track.measurement(j).uv, np.array(w["uv"]))


def test_run_index_error_past_keypoints():
    from gtsfm_amd.common.keypoints import Keypoints
    from gtsfm_amd.data_association.dsf_tracks_estimator import DsfTracksEstimator

    matches, coords, _ = ref.load_golden("dummy_matches")
    matches[(0, 3)] = np.array([[0, 5]])  # image 3 has keypoints 0..4
    with pytest.raises(IndexError):
        DsfTracksEstimator().run(matches, [Keypoints(c) for c in coords])


# ---- deep chains ----

@pytest.mark.parametrize("order", ["descending", "ascending", "shuffled"])
def test_chain(order):
    """One track across 200 images: (i, k_i) -- (i + 1, k_{i+1}). Descending image order hooks every root under a
    smaller one in turn, the deepest chains the union can see; the single track must not depend on the order."""
    n_img, kmax = 200, 7
    ks = np.random.default_rng(3).integers(0, kmax, n_img)
    idx = np.arange(n_img - 1)
    if order == "descending":
        idx = idx[::-1]
    elif order == "shuffled":
        idx = np.random.default_rng(4).permutation(idx)
    scene = _scene_of_rows([(i, i + 1) for i in idx], [[(ks[i], ks[i + 1])] for i in idx], n_img, kmax)
    got = _gpu(scene)
    want = _reference(scene)
    assert want.stats.tolist() == [1, n_img, 1, 0, 0]
    _compare(got, want, f"chain/{order}")
    np.testing.assert_array_equal(got[1][:n_img], np.arange(n_img))
    np.testing.assert_array_equal(got[2][:n_img], ks)


def test_chain_in_one_pair_list():
    """The same chain with all its rows in ONE launch-wide run of rows of pairs listed descending, every row twice:
    consecutive lanes of a wave extend one chain at the same time."""
    n_img, kmax = 200, 3
    idx = np.arange(n_img - 1)[::-1]
    scene = _scene_of_rows([(i + 1, i) for i in idx], [[(1, 2), (1, 2)] if i % 2 else [(2, 1), (2, 1)] for i in idx],
                           n_img, kmax)
    want = _reference(scene)
    assert want.stats[0] == 1 and want.stats[1] == n_img
    _compare(_gpu(scene), want, "chain/one-list")


# ---- contention on one root ----

def test_giant_invalid():
    """4 images x 3000 keypoints. Rows fuse 6,000 nodes of images 0 and 1 into one component (a path through both
    images plus random chords, so thousands of lanes hook onto and compress toward one root): 0 tracks from it and
    n_erroneous == 1. Four clean tracks in images 2, 3 and the unused tail of 0 and 1 survive."""
    n_img, kmax, big = 4, 3000, 2900
    rng = np.random.default_rng(5)
    k = np.arange(big)
    rows01 = np.concatenate([np.stack([k, k], 1), np.stack([k[1:], k[:-1]], 1),
                             rng.integers(0, big, (4000, 2))])
    rows01 = rows01[rng.permutation(len(rows01))]
    clean23 = np.array([[0, 5], [7, 7], [2999, 0]])
    clean02 = np.array([[2950, 0], [2960, 7]])   # joins tracks of (2, 3): (0,2950)-(2,0)-(3,5), (0,2960)-(2,7)-(3,7)
    clean13 = np.array([[2999, 2999]])
    scene = _scene_of_rows([(0, 1), (2, 3), (0, 2), (1, 3), (1, 0)],
                           [rows01, clean23, clean02, clean13, rows01[:1000, ::-1]], n_img, kmax)
    want = _reference(scene)
    assert want.stats.tolist() == [4, 10, 5, 1, 0]
    _compare(_gpu(scene), want, "giant_invalid")


# ---- duplicates, masks, bad rows ----

def test_dups_and_masks():
    base = ref.make_scene(12, 40, n_points=60, vis_prob=0.5, wrong_share=0.02, seed=7)
    P = len(base.pairs)
    rng = np.random.default_rng(8)
    valid = (rng.random(P) >= 0.3).astype(np.uint8)
    counts = np.diff(base.offsets)
    rows = [base.v_corr[base.offsets[p]: base.offsets[p + 1]] for p in range(P)]
    # rows of masked pairs that WOULD merge tracks: a full bipartite run between keypoints 0..5 of the two images
    for p in np.flatnonzero(valid == 0):
        rows[p] = np.concatenate([rows[p], np.stack(np.meshgrid(np.arange(6), np.arange(6)), -1).reshape(-1, 2)])
    pairs = base.pairs.copy()
    flip = rng.random(P) < 0.5  # i1 > i2
    pairs[flip] = pairs[flip][:, ::-1]
    rows = [r[:, ::-1] if f else r for r, f in zip(rows, flip)]
    rows = [np.concatenate([r, r]) for r in rows]  # every row twice
    pairs = np.concatenate([pairs, pairs[:5]])  # pairs listed twice
    rows = rows + rows[:5]
    valid = np.concatenate([valid, valid[:5]])
    kp_count = np.full(12, 40, np.int32)
    kp_count[3], kp_count[9] = 31, 0  # rows naming keypoints >= these counts are bad rows
    scene = _scene_of_rows(pairs, rows, 12, 40, valid=valid, kp_count=kp_count)
    # plus rows past kmax and an image index out of range, in valid pairs
    extra = _scene_of_rows(np.concatenate([scene.pairs, [[0, 1], [2, 12], [-1, 4]]]),
                           [scene.v_corr[scene.offsets[p]: scene.offsets[p + 1]] for p in range(len(scene.pairs))]
                           + [[(40, 0), (0, 40), (2 ** 31 - 1, 1)], [(0, 0)], [(1, 1)]], 12, 40,
                           valid=np.concatenate([scene.valid, [1, 1, 1]]), kp_count=kp_count)
    extra.v_corr[-5, 0] = -1  # 0xffffffff as the kernel reads it
    want = _reference(extra)
    assert want.stats[4] > 5 and want.stats[0] > 0 and want.stats[3] > 0 and (valid == 0).sum() > 5
    unmasked = ref.reference_tracks(extra.pairs, extra.offsets, extra.v_corr, kp_count, 40, None, None)
    assert unmasked.stats[0] != want.stats[0], "the masked rows must matter"
    _compare(_gpu(extra), want, "dups_and_masks")
    # the added bad rows have no other effect: without them the tracks are the same
    clean = ref.reference_tracks(scene.pairs, scene.offsets, scene.v_corr, kp_count, 40, scene.valid, scene.kp_xy)
    np.testing.assert_array_equal(clean.stats[:4], want.stats[:4])


# ---- edges of the launch ----

def test_zero_pairs_and_zero_rows():
    empty = _scene_of_rows(np.zeros((0, 2)), [], 3, 4)
    got = _gpu(empty)
    assert got[4].tolist() == [0, 0, 0, 0, 0] and got[0][0] == 0
    no_rows = _scene_of_rows([(0, 1), (1, 2)], [[], []], 3, 4)
    got = _gpu(no_rows)
    assert got[4].tolist() == [0, 0, 0, 0, 0] and got[0][0] == 0
    from gtsfm_amd.data_association.dsf_tracks_estimator import DsfTracksEstimator

    out = DsfTracksEstimator().run_arrays(empty.pairs, empty.offsets, empty.v_corr, empty.kp_count, 4)
    assert out.offsets.tolist() == [0] and len(out.image) == 0 and out.uv is None


@pytest.mark.parametrize("n_rows", [1, 255, 256, 257, 65537])
def test_row_counts(n_rows):
    """Rows spread over 40 pairs of 9 images; sizes around one workgroup and past one pass of the union grid."""
    rng = np.random.default_rng(n_rows)
    n_img, kmax = 9, 9000
    pairs = [(a, b) for a in range(n_img) for b in range(a + 1, n_img)] + [(1, 0), (2, 2), (0, 1), (8, 3)]
    cuts = np.sort(rng.integers(0, n_rows + 1, len(pairs) - 1))
    counts = np.diff(np.concatenate([[0], cuts, [n_rows]]))
    # latent points: row (point's keypoint in i1, in i2), keypoint = point id, with a few wrong ones
    rows = []
    for c in counts:
        pt = rng.integers(0, kmax, c)
        other = np.where(rng.random(c) < 0.002, rng.integers(0, kmax, c), pt)
        rows.append(np.stack([pt, other], 1))
    scene = _scene_of_rows(pairs, rows, n_img, kmax)
    _compare(_gpu(scene), _reference(scene), f"rows{n_rows}")


def test_empty_pair_in_the_middle_and_no_xy():
    scene = _scene_of_rows([(0, 1), (0, 2), (1, 2), (2, 3), (1, 3)],
                           [[(0, 0), (1, 1)], [], [(0, 5)], [], [(1, 2), (3, 3)]], 4, 6)
    want = _reference(scene)
    assert want.stats.tolist() == [3, 8, 3, 0, 0]
    got = _gpu(scene, kp_xy=False)
    assert got[3] is None
    _compare(got, want, "empty pair, no xy")
    _compare(_gpu(scene), want, "empty pair")


def test_oversized_row_buffer_is_not_read():
    """v_corr larger than offsets[P] (compact_verified's `capacity`): the tail is ignored."""
    scene = _scene_of_rows([(0, 1), (1, 2)], [[(0, 0), (1, 1)], [(0, 0)]], 3, 4)
    want = _reference(scene)
    padded = scene._replace(v_corr=np.concatenate([scene.v_corr, np.full((300, 2), 2, np.int32)]))
    _compare(_gpu(padded), want, "padded v_corr")


# ---- the large scene ----

def test_scene300():
    scene, want = _scene300()
    n_tracks, n_meas, n_comp, n_err, n_bad = want.stats.tolist()
    lengths = want.track_lengths()
    print(f"scene300: {len(scene.v_corr)} rows, stats {want.stats.tolist()}, longest track {lengths.max()}")
    # conditions on the seeded input
    assert len(scene.v_corr) > 2048 * 256  # more than one pass of the union kernel's grid
    assert 0 < n_err < n_comp
    assert (lengths >= 20).any() and (lengths == 2).any()
    _compare(_gpu(scene), want, "scene300")


def test_determinism_under_row_order():
    scene, want = _scene300()
    a = _gpu(ref.shuffle_rows(scene, 11))
    b = _gpu(ref.shuffle_rows(scene, 12))
    n_tracks, n_meas = int(want.stats[0]), int(want.stats[1])
    for x, y, n in zip(a, b, (n_tracks + 1, n_meas, n_meas, n_meas, 5)):
        assert x[:n].tobytes() == y[:n].tobytes()
    _compare(a, want, "scene300 shuffled")


def test_capacity():
    """Short capacities: nothing is written past them (canaries intact) and stats carry the true counts."""
    scene, want = _scene300()
    n_tracks, n_meas = int(want.stats[0]), int(want.stats[1])
    track_cap, meas_cap = n_tracks // 2, n_meas // 3
    dev = torch.device(DEV)
    pad = 64
    t_off = torch.full((track_cap + 1 + pad,), -7, dtype=torch.int32, device=dev)
    t_img = torch.full((meas_cap + pad,), -7, dtype=torch.int32, device=dev)
    t_kp = torch.full((meas_cap + pad,), -7, dtype=torch.int32, device=dev)
    t_uv = torch.full((meas_cap + pad, 2), -7.0, dtype=torch.float32, device=dev)
    got = _gpu(scene, track_cap=track_cap, meas_cap=meas_cap, out=(t_off, t_img, t_kp, t_uv))
    np.testing.assert_array_equal(got[4], want.stats)
    np.testing.assert_array_equal(got[0][: track_cap + 1], want.offsets[: track_cap + 1])
    np.testing.assert_array_equal(got[1][:meas_cap], want.image[:meas_cap])
    np.testing.assert_array_equal(got[2][:meas_cap], want.keypoint[:meas_cap])
    assert got[3][:meas_cap].tobytes() == want.uv[:meas_cap].tobytes()
    assert (got[0][track_cap + 1:] == -7).all() and (got[1][meas_cap:] == -7).all()
    assert (got[2][meas_cap:] == -7).all() and (got[3][meas_cap:] == -7.0).all()


def test_bad_arguments():
    from gtsfm_amd import native

    L = native.lib()
    dev = torch.device(DEV)
    buf = torch.zeros(1 << 16, dtype=torch.int32, device=dev)
    p = buf.data_ptr()
    ok_ws = L.gtsfm_tracks_workspace_bytes(3, 4, 1, 2)
    assert 0 < ok_ws <= buf.numel() * 4

    def call(n_pairs=1, n_rows=2, n_img=3, kmax=4, ws=p, ws_bytes=ok_ws, pairs=p, stats=p, track_cap=8, meas_cap=8):
        return L.gtsfm_tracks_from_matches(pairs, p, p, None, n_pairs, n_rows, p, None, n_img, kmax, ws, ws_bytes, p,
                                           track_cap, p, p, None, meas_cap, stats, None)

    assert call(n_pairs=-1) == native.GTSFM_ERR_ARG
    assert call(n_rows=-1) == native.GTSFM_ERR_ARG
    assert call(ws_bytes=ok_ws - 1) == native.GTSFM_ERR_ARG
    assert call(ws=None) == native.GTSFM_ERR_ARG
    assert call(pairs=None) == native.GTSFM_ERR_ARG
    assert call(stats=None) == native.GTSFM_ERR_ARG
    assert call(n_img=1 << 16, kmax=1 << 15) == native.GTSFM_ERR_ARG  # n_img * kmax == 2^31
    assert call(track_cap=-1) == native.GTSFM_ERR_ARG
    torch.cuda.synchronize()


# ---- chained to the front-end's outputs, on the device ----

def test_chained_to_viewgraph_keep():
    """A compact_verified-shaped CSR (int32 tensors holding uint32, a row buffer larger than its contents) and the
    view-graph filter's keep, combined with isp_ok on the device, go straight into run_arrays: no host copy between
    the two calls. The result equals the restatement on the dict of the pairs that survive."""
    import viewgraph_ref as vref
    from gtsfm_amd.data_association.dsf_tracks_estimator import DsfTracksEstimator
    from gtsfm_amd.view_graph_estimator.cycle_consistent_rotation_estimator import (
        CycleConsistentRotationViewGraphEstimator, EdgeErrorAggregationCriterion)

    n_img = 20
    pairs, R = vref.make_scene(n_img, seed=9, outlier_share=0.25)  # complete graph, (i1, i2) order
    scene = ref.make_scene(n_img, 64, n_points=150, vis_prob=0.3, wrong_share=0.01, seed=9)
    np.testing.assert_array_equal(pairs, scene.pairs)
    dev = torch.device(DEV)
    isp_ok = (np.random.default_rng(10).random(len(pairs)) > 0.2).astype(np.uint8)
    pairs_d = torch.from_numpy(pairs).to(dev)
    v_corr_d = torch.zeros((len(scene.v_corr) + 100, 2), dtype=torch.int32, device=dev)
    v_corr_d[: len(scene.v_corr)] = torch.from_numpy(scene.v_corr).to(dev)
    keep_d, _, _ = CycleConsistentRotationViewGraphEstimator(EdgeErrorAggregationCriterion.MEDIAN_EDGE_ERROR).run_arrays(
        pairs_d, torch.from_numpy(R).to(dev), num_images=n_img)
    valid_d = keep_d & (torch.from_numpy(isp_ok).to(dev) != 0)
    got = DsfTracksEstimator().run_arrays(pairs_d, torch.from_numpy(scene.offsets).to(dev), v_corr_d,
                                          torch.from_numpy(scene.kp_count).to(dev), scene.kmax, valid=valid_d,
                                          kp_xy=torch.from_numpy(scene.kp_xy).to(dev))
    assert all(a.is_cuda for a in got)
    valid = valid_d.cpu().numpy()
    assert 0 < valid.sum() < len(valid) and (valid != (isp_ok != 0)).any()
    filtered = ref.scene_as_dict(scene._replace(valid=valid.astype(np.uint8)))
    f_pairs, f_offsets, f_rows = ref.csr_from_dict(filtered)
    want = ref.reference_tracks(f_pairs, f_offsets, f_rows, scene.kp_count, scene.kmax, None, scene.kp_xy)
    assert want.stats[0] > 0
    _compare([a.cpu().numpy() for a in got], want, "chained")
