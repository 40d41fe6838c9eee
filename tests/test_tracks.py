"""CPU side of the track estimator: the restatement against the reference's known answers, the track types, the ABI
surface and the host-side validation. Nothing here needs a GPU.

The first block pins tests/tracks_ref.py (the yardstick of tests/test_tracks_gpu.py) to the cases of the reference's
tests/data_association/test_dsf_tracks_estimator.py, stored as data under tests/golden/tracks/; it passes without the
feature. Everything after it needs the feature.
"""
import numpy as np
import pytest

import tracks_ref as ref


# ---- the restatement reproduces the reference's known answers ----

@pytest.mark.parametrize("name", ref.GOLDEN_CASES)
def test_restatement_track_counts(name):
    matches, coords, case = ref.load_golden(name)
    got = ref.reference_tracks_from_dict(matches, coords)
    assert got.stats[0] == case["n_tracks"] == len(got.offsets) - 1
    assert got.stats[1] == len(got.image) == len(got.keypoint) == got.offsets[-1]
    assert got.stats[2] - got.stats[3] == got.stats[0]


def test_restatement_three_images_index_wise():
    matches, coords, case = ref.load_golden("three_images")
    got = ref.reference_tracks_from_dict(matches, coords)
    for t, want in enumerate(case["tracks"]):
        lo, hi = got.offsets[t], got.offsets[t + 1]
        assert got.image[lo:hi].tolist() == [m["i"] for m in want]
        np.testing.assert_array_equal(got.uv[lo:hi], np.array([m["uv"] for m in want], np.float32))


def test_restatement_malformed_and_nontransitive_components():
    matches, coords, _ = ref.load_golden("malformed_same_image")
    assert ref.reference_tracks_from_dict(matches, coords).stats.tolist() == [4, 9, 5, 1, 0]
    matches, coords, _ = ref.load_golden("nontransitive")
    assert ref.reference_tracks_from_dict(matches, coords).stats.tolist() == [0, 0, 1, 1, 0]


def test_restatement_against_a_plain_union_find():
    """The scipy route and a row-by-row union-find (the reference's loop, dsf_tracks_estimator.py:56-85) agree on a
    seeded scene with wrong rows, masked pairs and shuffled rows."""
    scene = ref.make_scene(15, 30, n_points=80, vis_prob=0.4, wrong_share=0.03, masked_share=0.3, shuffle=True, seed=2)
    got = ref.reference_tracks(scene.pairs, scene.offsets, scene.v_corr, scene.kp_count, scene.kmax, scene.valid)
    parent = {}

    def find(x):
        parent.setdefault(x, x)
        while parent[x] != x:
            x = parent[x]
        return x

    for p, (i1, i2) in enumerate(scene.pairs):
        if not scene.valid[p]:
            continue
        for k1, k2 in scene.v_corr[scene.offsets[p]: scene.offsets[p + 1]]:
            a, b = find((int(i1), int(k1))), find((int(i2), int(k2)))
            if a != b:
                parent[max(a, b)] = min(a, b)
    sets = {}
    for node in parent:
        sets.setdefault(find(node), []).append(node)
    tracks = [sorted(s) for s in sets.values() if len({i for i, _ in s}) == len(s)]
    tracks.sort(key=lambda s: s[0])
    assert got.stats.tolist() == [len(tracks), sum(map(len, tracks)), len(sets), len(sets) - len(tracks), 0]
    assert 0 < got.stats[3] < got.stats[2]
    flat = [node for s in tracks for node in s]
    assert list(zip(got.image.tolist(), got.keypoint.tolist())) == flat


def test_scene_maker_shuffle_keeps_the_rows():
    scene = ref.make_scene(8, 20, n_points=40, vis_prob=0.5, wrong_share=0.05, masked_share=0.2, seed=3)
    other = ref.shuffle_rows(scene, 5)
    assert not np.array_equal(scene.pairs, other.pairs)
    a = ref.reference_tracks(*scene[:5], scene.valid, scene.kp_xy)
    b = ref.reference_tracks(*other[:5], other.valid, other.kp_xy)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


# ---- SfmTrack2d / SfmMeasurement ----

def _track():
    from gtsfm_amd.common.sfm_track import SfmMeasurement, SfmTrack2d

    return SfmTrack2d([SfmMeasurement(0, np.array([10.0, 20.0])), SfmMeasurement(3, np.array([30.0, 40.0])),
                       SfmMeasurement(5, np.array([50.0, 60.0]))])


def test_sfm_track_accessors_and_subsets():
    from gtsfm_amd.common.sfm_track import SfmMeasurement, SfmTrack2d

    track = _track()
    assert track.number_measurements() == 3
    assert track.measurement(1).i == 3 and track.measurement(1).uv.tolist() == [30.0, 40.0]
    sub = track.select_subset([2, 0])
    assert [m.i for m in sub.measurements] == [5, 0]
    with pytest.raises(IndexError):
        track.select_subset([3])
    cams = track.select_for_cameras({3, 5, 9})  # 9 has no measurement here: not an error
    assert [m.i for m in cams.measurements] == [3, 5]
    assert track.validate_unique_cameras()
    twice = SfmTrack2d(track.measurements + [SfmMeasurement(3, np.array([1.0, 2.0]))])
    assert not twice.validate_unique_cameras()


def test_sfm_track_equality_ignores_order():
    from gtsfm_amd.common.sfm_track import SfmMeasurement, SfmTrack2d

    track = _track()
    assert track == SfmTrack2d(track.measurements[::-1])
    assert not track != SfmTrack2d(track.measurements[::-1])
    assert track != SfmTrack2d(track.measurements[:2])
    moved = SfmTrack2d(track.measurements[:2] + [SfmMeasurement(5, np.array([50.0, 61.0]))])
    assert track != moved
    assert SfmMeasurement(1, np.array([1.0, 2.0])) == SfmMeasurement(1, np.array([1.0, 2.0 + 1e-12]))
    assert SfmMeasurement(1, np.array([1.0, 2.0])) != SfmMeasurement(2, np.array([1.0, 2.0]))
    assert track != "track" and SfmMeasurement(1, np.zeros(2)) != (1, np.zeros(2))


# ---- ABI surface ----

def test_signatures_list_both_entry_points_with_the_headers_arity():
    from gtsfm_amd import native
    from tests.test_integration_doc import _header_arity

    arity = _header_arity()
    for name in ("gtsfm_tracks_workspace_bytes", "gtsfm_tracks_from_matches"):
        assert name in native.SIGNATURES and name in arity
        assert len(native.SIGNATURES[name][1]) == arity[name]
    assert arity["gtsfm_tracks_workspace_bytes"] == 4
    assert native.ABI_VERSION >= 404


def test_workspace_query():
    from gtsfm_amd import native

    q = native.lib().gtsfm_tracks_workspace_bytes
    for empty in ((0, 2048, 10, 100), (1000, 0, 10, 100), (1000, 2048, 0, 100), (1000, 2048, 10, 0),
                  (-1, 2048, 10, 100), (1000, 2048, 10, -5)):
        assert q(*empty) == 0, empty
    assert q(1 << 16, 1 << 15, 10, 100) == 0  # n_img * kmax == 2^31: unsupported
    assert q(1000, 2048, 10, 1 << 31) == 0
    sizes = [q(1000, 2048, 499500, rows) for rows in (1, 1000, 10 ** 6, 5 * 10 ** 7, 2 ** 31 - 1)]
    assert sizes[0] > 0 and sizes == sorted(sizes)
    assert q(1000, 2048, 499500, 10 ** 6) >= 1000 * 2048 * 4  # at least the parent array
    assert q(2000, 2048, 10, 100) > q(1000, 2048, 10, 100)


# ---- host-side validation of run() ----

def test_run_rejects_rank1_coordinates_before_the_gpu(monkeypatch):
    """test_cpp_dsf_tracks_estimator.py:16-22: coordinates of shape (2,) raise ValueError; no GPU is needed for it."""
    from gtsfm_amd import native
    from gtsfm_amd.common.keypoints import Keypoints
    from gtsfm_amd.data_association.dsf_tracks_estimator import CppDsfTracksEstimator, DsfTracksEstimator
    from gtsfm_amd.data_association.tracks_estimator_base import TracksEstimatorBase

    def no_gpu():
        raise AssertionError("run() reached the GPU before validating its inputs")

    monkeypatch.setattr(native, "require_gpu", no_gpu)
    assert issubclass(DsfTracksEstimator, TracksEstimatorBase) and CppDsfTracksEstimator is DsfTracksEstimator
    matches = {(0, 1): np.array([[0, 0]])}
    kps = [Keypoints(np.array([1.0, 2.0])), Keypoints(np.array([[1.0, 2.0]]))]
    with pytest.raises(ValueError):
        CppDsfTracksEstimator().run(matches, kps)
    with pytest.raises(IndexError):
        DsfTracksEstimator().run({(0, 1): np.array([[0, 1]])}, [Keypoints(np.zeros((1, 2))), Keypoints(np.zeros((1, 2)))])
    with pytest.raises(IndexError):
        DsfTracksEstimator().run({(0, 2): np.array([[0, 0]])}, [Keypoints(np.zeros((1, 2))), Keypoints(np.zeros((1, 2)))])
    assert DsfTracksEstimator().run({}, kps[1:]) == []
