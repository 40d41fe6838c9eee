"""D2NetDetDesc + TwoWayMatcher through DetDescCorrespondenceGenerator's batched device path ('d2net_twoway').

Bar: generate_correspondences returns what the per-call route returns (detect_and_describe per image, then
TwoWayMatcher.match per pair): keypoint coordinates and responses bit-equal, match arrays equal; also with both
cachers, on a cold, a warm and a half-populated cache directory. Seeded random weights (tests/d2net_weights.py);
4 images of two shapes, 48 x 64 (an 11 x 15 map, the smallest in tests/test_d2net_gpu.py, ~80 detections) and
100 x 140; the second image of each shape is the first rolled by whole map cells, so a ratio test keeps matches.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from d2net_weights import d2net_state_dict, textured_image  # noqa: E402

pytestmark = pytest.mark.gpu

K = 60
PAIRS = [(0, 1), (2, 3), (0, 2), (3, 1), (1, 0)]


@pytest.fixture(scope="module")
def detector():
    from gtsfm_amd import native
    from gtsfm_amd.frontend.detector_descriptor.d2net import D2NetDetDesc

    native.require_gpu()
    return D2NetDetDesc(max_keypoints=K, state_dict=d2net_state_dict(0))


@pytest.fixture(scope="module")
def images():
    from gtsfm_amd.common.image import Image

    a, c = textured_image(10, 48, 64), textured_image(11, 100, 140)
    return [Image(a), Image(np.roll(a, 4, axis=1)), Image(c), Image(np.roll(c, 8, axis=0))]


@pytest.fixture(scope="module")
def per_call(detector, images):
    """The per-call route, computed once and left unchanged: (features per image, matches per pair)."""
    from gtsfm_amd.frontend.matcher.twoway_matcher import TwoWayMatcher

    feats = [detector.detect_and_describe(im) for im in images]
    matcher = TwoWayMatcher(ratio_test_threshold=0.8)
    corr = {(i1, i2): matcher.match(feats[i1][0], feats[i2][0], feats[i1][1], feats[i2][1], images[i1].shape,
                                    images[i2].shape) for i1, i2 in PAIRS}
    assert min(len(kp) for kp, _ in feats) > 8
    assert len(corr[(0, 1)]) > 0 and len(corr[(2, 3)]) > 0
    return feats, corr


def same(result, per_call):
    kps, corr = result
    feats, ref = per_call
    assert len(kps) == len(feats)
    for kp, (rkp, _) in zip(kps, feats):
        assert kp.coordinates.dtype == rkp.coordinates.dtype and kp.responses.dtype == rkp.responses.dtype
        assert np.array_equal(kp.coordinates, rkp.coordinates)
        assert np.array_equal(kp.responses, rkp.responses)
        assert kp.scales is None and rkp.scales is None
    assert list(corr) == PAIRS
    for key in PAIRS:
        assert corr[key].shape == ref[key].shape and corr[key].dtype == ref[key].dtype, key
        assert np.array_equal(corr[key], ref[key]), key


def generator(detector, cache_root=None):
    from gtsfm_amd.frontend.cacher.detector_descriptor_cacher import DetectorDescriptorCacher
    from gtsfm_amd.frontend.cacher.matcher_cacher import MatcherCacher
    from gtsfm_amd.frontend.correspondence_generator.det_desc_correspondence_generator import (
        DetDescCorrespondenceGenerator)
    from gtsfm_amd.frontend.matcher.twoway_matcher import TwoWayMatcher

    matcher = TwoWayMatcher(ratio_test_threshold=0.8)
    if cache_root is None:
        return DetDescCorrespondenceGenerator(matcher, detector)
    return DetDescCorrespondenceGenerator(MatcherCacher(matcher, cache_root=cache_root),
                                          DetectorDescriptorCacher(detector, cache_root=cache_root))


def test_batched_path_equals_per_call(detector, images, per_call):
    gen = generator(detector)
    assert gen._batched() == "d2net_twoway"
    same(gen.generate_correspondences(None, images, PAIRS), per_call)
    f = gen.device_features
    assert f.desc.shape == (4, K, 512) and f.desc.is_cuda
    cnt = f.count.cpu().numpy()
    for i, (_, desc) in enumerate(per_call[0]):
        assert np.array_equal(f.desc[i, : cnt[i]].cpu().numpy(), desc)


def test_with_cachers_cold_and_warm(detector, images, per_call, tmp_path):
    gen = generator(detector, tmp_path)
    assert gen._batched() == "d2net_twoway"
    same(gen.generate_correspondences(None, images, PAIRS), per_call)  # populates the cache
    assert len(list((tmp_path / "detector_descriptor").iterdir())) == 4
    assert len(list((tmp_path / "matcher").iterdir())) == len(PAIRS)
    gen = generator(detector, tmp_path)
    same(gen.generate_correspondences(None, images, PAIRS), per_call)  # every image and pair from the cache
    assert gen.device_features.desc.shape[2] == 512 and getattr(gen.device_features, "from_host", False)


def test_with_half_populated_cache(detector, images, per_call, tmp_path):
    """Images 0 and 2 and the pair between them are cached, the rest is not: the block merges cache hits
    (features_from_host at 512-D) with batched misses."""
    feats, corr = per_call
    kps, sub = generator(detector, tmp_path).generate_correspondences(None, [images[0], images[2]], [(0, 1)])
    assert np.array_equal(kps[1].coordinates, feats[2][0].coordinates) and np.array_equal(sub[(0, 1)], corr[(0, 2)])
    assert len(list((tmp_path / "detector_descriptor").iterdir())) == 2
    gen = generator(detector, tmp_path)
    same(gen.generate_correspondences(None, images, PAIRS), per_call)
    assert gen.device_features.desc.shape[2] == 512
    assert len(list((tmp_path / "detector_descriptor").iterdir())) == 4
