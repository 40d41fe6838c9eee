"""CPU checks of the LightGlue restatement (tests/lightglue_ref.py), the planted weights and the weight packing.

The float64 restatement is the oracle of tests/test_lightglue_gpu.py. Here: its float32 form stays within the
recorded distance of it on every GPU case (lightglue_cases.MEASURED, from which the GPU bars derive); the rotary
convention is pinned by translation invariance; the planted exit layers are what the weights promise and every stop
decision is robust, so that the GPU comparison of exit layers can be exact.
"""
import pickle

import numpy as np
import pytest

import lightglue_cases as lc
import lightglue_ref
import lightglue_weights as lgw
from gtsfm_amd.common.keypoints import Keypoints
from gtsfm_amd.frontend.matcher.lightglue_matcher import (LightGlueMatcher, pack_lightglue_weights, qkv_permutation)


@pytest.mark.parametrize("name", sorted(lc.MEASURED))
def test_float32_stays_within_the_recorded_distance(name):
    a, b = lc.cases()[name]
    r64, r32 = lc.reference_of(name), lc.reference(a, b, dtype="float32")
    live = r64.Z > -20
    dz = float(np.abs(r32.Z - r64.Z)[live].max())
    ds = float(np.abs(r32.mscores0 - r64.mscores0).max())
    differ = int((r32.matches0 != r64.matches0).sum())
    print(f'    "{name}": ({dz:.2e}, {ds:.2e}, {differ}, {len(r64.matches)}),')
    rec = lc.MEASURED[name]
    # The record holds what one machine measured; another BLAS or thread count sums in another order, and a small
    # case's figure moves by more than its own size. What must hold everywhere is that the float32 restatement itself
    # meets the bars the GPU is held to (4 x the recorded maxima over all cases).
    zbar, sbar = lc.bars()
    assert dz <= zbar and ds <= sbar, (dz, ds, rec)
    assert len(r64.matches) == rec[3]
    assert differ <= max(2, 0.02 * len(r64.matches))
    assert r32.exit_layer == r64.exit_layer
    assert (r32.Z[~live] < -15).all()


def test_cases_cover_the_measured_table():
    assert sorted(lc.cases()) == sorted(lc.MEASURED)


def test_translation_leaves_the_assignment_unchanged():
    """Rotary encoding reaches the scores only through relative phases, so shifting all of one image's keypoints
    leaves Z unchanged in float64. A rot / repeat convention that does not match (pairs (2j, 2j + 1) sharing
    frequency j) breaks this."""
    a, b = lc.cases()["65x127"]
    ref = lc.reference_of("65x127")
    # (the shift is made in float64: in float32 the moved keypoints would round, which is no translation)
    moved = lc.reference(a._replace(kp=a.kp.astype(np.float64) + [37.0, -21.0]), b)
    assert np.abs(moved.Z - ref.Z).max() < 1e-9
    moved = lc.reference(a, b._replace(kp=b.kp.astype(np.float64) + [-8.0, 64.0]))
    assert np.abs(moved.Z - ref.Z).max() < 1e-9
    # and the positions matter at all: moving one keypoint alone changes Z
    kp = a.kp.copy()
    kp[0] += 50.0
    assert np.abs(lc.reference(a._replace(kp=kp), b).Z - ref.Z).max() > 1e-4


def test_zero_Wr_is_the_network_without_the_rotary_step():
    a, b = lc.cases()["15x17"]
    sd = dict(lc.state_dict())
    sd["posenc.Wr.weight"] = np.zeros((32, 2), np.float32)
    with_zero = lc.reference(a, b, sd=sd)
    without = lc.reference(a, b, sd=sd, rotary=False)
    np.testing.assert_allclose(with_zero.Z, without.Z, rtol=0, atol=1e-12)
    assert np.abs(with_zero.Z - lc.reference_of("15x17").Z).max() > 1e-4


def _robust(decisions):
    for below, near, total, stopped in decisions:
        assert stopped == (below < 0.05 * total)
        assert near < abs(below - 0.05 * total), (below, near, total)


def test_planted_exit_layers_and_robust_decisions():
    exits = [lc.reference_of(f"depth_{i}_{j}").exit_layer for i, j in lc.DEPTH_PAIRS]
    assert len(set(exits)) >= 3 and 0 in exits and 8 in exits, exits
    assert lgw.LATE_LAYER in exits
    for name in lc.MEASURED:
        r = lc.reference_of(name)
        _robust(r.decisions)
        assert len(r.decisions) == min(r.exit_layer + 1, 8)


def test_wrong_layers_assignment_weights_give_another_answer():
    zbar, _ = lc.bars()
    a, b = lc.cases()["depth_0_1"]
    ref = lc.reference_of("depth_0_1")
    assert ref.exit_layer == 0
    wrong = lc.reference(a, b, assign_layer=8)
    live = ref.Z > -20
    assert np.abs(wrong.Z - ref.Z)[live].max() > 100 * zbar


def test_stopping_disabled_runs_every_layer():
    r = lc.reference_of("depth_0_1", depth_confidence=-1.0)
    assert r.exit_layer == 8 and r.decisions == []
    assert np.abs(r.Z - lc.reference_of("depth_0_1").Z).max() > 1e-3


def test_identical_columns_match_the_lower_index():
    a, b, lo, hi = lc.make_tie_pair()
    r = lc.reference(a, b)
    np.testing.assert_array_equal(r.Z[:, lo], r.Z[:, hi])
    assert lo in r.matches[:, 1] and hi not in r.matches[:, 1]


def test_weight_blob_layout():
    from gtsfm_amd import native

    sd = lc.state_dict()
    blob = pack_lightglue_weights(sd)
    assert blob.dtype == np.float32 and blob.size == native.lib().gtsfm_lightglue_weights_floats(9)
    np.testing.assert_array_equal(blob[:64].reshape(32, 2), sd["posenc.Wr.weight"])
    # Wqkv^T (256 x 768) follows: column s * 256 + h * 64 + e <- upstream output channel h * 192 + e * 3 + s
    perm = qkv_permutation()
    assert sorted(perm.tolist()) == list(range(768))
    assert perm[0] == 0 and perm[1] == 3 and perm[64] == 192 and perm[256] == 1 and perm[512 + 64 + 5] == 192 + 15 + 2
    wt = blob[64: 64 + 256 * 768].reshape(256, 768)
    W = sd["transformers.0.self_attn.Wqkv.weight"]
    for s, h, e in ((0, 0, 0), (1, 2, 7), (2, 3, 63)):
        np.testing.assert_array_equal(wt[:, s * 256 + h * 64 + e], W[h * 192 + e * 3 + s])
    bias = blob[64 + 256 * 768: 64 + 256 * 768 + 768]
    assert bias[256 + 2 * 64 + 7] == sd["transformers.0.self_attn.Wqkv.bias"][2 * 192 + 7 * 3 + 1]
    # the last layer's tail: final_proj, bias, matchability w, token w (none: zeros), matchability b, token b
    tail = blob[-(256 * 256 + 256 + 256 + 256 + 4):]
    np.testing.assert_array_equal(tail[: 256 * 256].reshape(256, 256), sd["log_assignment.8.final_proj.weight"].T)
    assert tail[256 * 256 + 768] == sd["log_assignment.8.matchability.bias"][0]
    assert not tail[256 * 256 + 512: 256 * 256 + 768].any()


def test_old_checkpoint_keys_give_the_same_blob():
    old = lgw.lightglue_state_dict(lc.WEIGHT_SEED, old_names=True)
    assert "self_attn.0.Wqkv.weight" in old and "confidence_thresholds" in old
    np.testing.assert_array_equal(pack_lightglue_weights(old), pack_lightglue_weights(lc.state_dict()))


def test_matcher_pickles_without_its_device_blob():
    m = LightGlueMatcher("superpoint", state_dict=lc.state_dict())
    m._blob = object()  # stands for the device tensor, which does not travel
    m2 = pickle.loads(pickle.dumps(m))
    assert m2._blob is None and m2._features == "superpoint"
    np.testing.assert_array_equal(m2._state_dict["posenc.Wr.weight"], lc.state_dict()["posenc.Wr.weight"])


def test_matcher_argument_checks():
    with pytest.raises(ValueError, match="input_proj"):
        LightGlueMatcher(features="disk")
    with pytest.raises(ValueError, match="scale and orientation"):
        LightGlueMatcher(features="sift")
    m = LightGlueMatcher("superpoint", state_dict=lc.state_dict())
    a, b = lc.cases()["15x17"]
    with pytest.raises(ValueError, match="Responses"):
        m.match(Keypoints(a.kp), Keypoints(b.kp, responses=b.scores), a.desc, b.desc, (*a.hw, 3), (*b.hw, 3))
