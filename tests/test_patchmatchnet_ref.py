"""PatchmatchNet without a GPU: the torch restatement (tests/patchmatchnet_ref.py) against the reference's recorded
outputs, the weight blob's layout, the workspace query, and the conditions the golden itself has to meet."""
import os

import numpy as np
import pytest
import torch

import patchmatchnet_ref as pref
from patchmatchnet_weights import patchmatchnet_state_dict
from tests.conftest import GOLDEN

CASES = ("a", "b")
OUTPUTS = ["iter0", "iter1", "iter2", "iter3", "iter4", "depth", "confidence"]


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "patchmatchnet_random_w0.npz")) as z:
        return {name: pref.load_golden_case(z, name) for name in CASES}


@pytest.fixture(scope="module")
def state_dict():
    return patchmatchnet_state_dict(0)


def _outputs(r):
    out = {f"iter{i}": d.numpy() for i, d in enumerate(r["iter_depths"])}
    out.update(depth=r["depth"].numpy(), confidence=r["confidence"].numpy())
    return out


@pytest.mark.parametrize("name", CASES)
def test_restatement_fp64_matches_reference_fp64(golden, state_dict, name):
    """Same arithmetic in the same precision: what is left is summation order, 1e-12 of values of order 1 to 10."""
    case = golden[name]
    r = pref.run_case(state_dict, case, torch.float64)
    for key, got in _outputs(r).items():
        np.testing.assert_allclose(got, case[f"{key}_f64"], rtol=0, atol=1e-10, err_msg=key)
    np.testing.assert_allclose(r["index"].numpy(), case["index_f64"], rtol=0, atol=1e-10)
    for stage in (1, 2, 3):
        want = case[f"feat{stage}"]  # stored as fp32
        assert np.abs(r["features"][stage][0].numpy() - want).max() <= 2e-7 * np.abs(want).max()


@pytest.mark.parametrize("name", CASES)
def test_restatement_fp32_matches_reference_fp32(golden, state_dict, name):
    """Two fp32 evaluations of one function differ by about what either differs from fp64: the restatement's distance
    from the reference's fp32 output may be at most 4 x the reference's own fp32 error (median and 99th percentile),
    the bound the HIP path is held to against fp64."""
    case = golden[name]
    r = pref.run_case(state_dict, case, torch.float32)
    span = float(case["depth_range"][0, 1] - case["depth_range"][0, 0])
    for key, got in _outputs(r).items():
        s = 1.0 if key == "confidence" else span
        ref = pref.error_figures(case[f"{key}_f32"], case[f"{key}_f64"], s)
        mine = pref.error_figures(got, case[f"{key}_f32"], s)
        print(name, key, "reference fp32 vs fp64", ref, "restatement fp32 vs reference fp32", mine)
        assert mine[0] <= 4 * ref[0] and mine[1] <= 4 * ref[1] and mine[2] <= ref[2] + 0.01, key
    for stage in (1, 2, 3):
        want = case[f"feat{stage}"]
        assert np.abs(r["features"][stage][0].numpy() - want).max() <= 2e-4 * np.abs(want).max()


@pytest.mark.parametrize("name", CASES)
def test_golden_is_not_degenerate(golden, name):
    """Conditions on the inputs the golden maker must meet, not tolerances on any kernel."""
    case = golden[name]
    span = float(case["depth_range"][0, 1] - case["depth_range"][0, 0])
    for key in OUTPUTS:
        assert np.isfinite(case[f"{key}_f32"]).all() and np.isfinite(case[f"{key}_f64"]).all()
    assert case["confidence_f64"].std() >= 0.02
    index = case["index_f64"]
    assert (np.abs(index - np.round(index)) < 1e-3).mean() <= 0.01
    assert (np.abs(case["depth_f32"] - case["depth_f64"]) > 1e-4 * span).mean() <= 0.01


def test_case_b_covers_padding_and_negative_depth(golden):
    """View 4 of case (b) stands inside view 0's depth range: some of view 0's hypotheses fall behind it (the negative
    depth rule) and some in front of it project outside its image (zero padding)."""
    case = golden["b"]
    projs = pref.projection_matrices(case["wRc"], case["wtc"], case["intrinsics"])[1]
    rel = projs[4] @ np.linalg.inv(projs[0])
    H, W = case["images"].shape[1] // 2, case["images"].shape[2] // 2
    ys, xs = np.mgrid[0:H, 0:W]
    behind = outside = inside = 0
    for depth in np.linspace(*case["depth_range"][0], 8):
        p = rel[:3, :3] @ np.stack((xs.ravel(), ys.ravel(), np.ones(H * W))) * depth + rel[:3, 3:4]
        neg = p[2] <= 1e-3
        u, v = p[0] / np.where(neg, 1, p[2]), p[1] / np.where(neg, 1, p[2])
        out = ~neg & ((u < 0) | (u > W - 1) | (v < 0) | (v > H - 1))
        behind, outside, inside = behind + neg.sum(), outside + out.sum(), inside + (~neg & ~out).sum()
    assert behind > 0 and outside > 0 and inside > 0


def test_blob_layout_and_size(state_dict):
    from gtsfm_amd import native
    from gtsfm_amd.densify import pack_patchmatchnet_weights

    blob = pack_patchmatchnet_weights(state_dict)
    assert blob.dtype == np.float32 and blob.size == native.lib().gtsfm_patchmatchnet_weights_floats()
    # feature.conv0 first: W[ky][kx][ci][co] = weight[co][ci][ky][kx] * gamma / sqrt(var + eps), then the folded bias
    sd = {k: np.asarray(v, np.float64) for k, v in state_dict.items()}
    scale = sd["feature.conv0.bn.weight"] / np.sqrt(sd["feature.conv0.bn.running_var"] + 1e-5)
    want = (sd["feature.conv0.conv.weight"] * scale[:, None, None, None]).transpose(2, 3, 1, 0)
    np.testing.assert_allclose(blob[: 9 * 3 * 8].reshape(3, 3, 3, 8), want, rtol=1e-6)
    shift = sd["feature.conv0.bn.bias"] - sd["feature.conv0.bn.running_mean"] * scale
    np.testing.assert_allclose(blob[9 * 3 * 8: 9 * 3 * 8 + 8], shift, rtol=1e-6, atol=1e-7)
    # the DataParallel prefix of the reference's checkpoint is accepted
    prefixed = pack_patchmatchnet_weights({f"module.{k}": v for k, v in state_dict.items()})
    np.testing.assert_array_equal(prefixed, blob)


def test_workspace_query_refuses_bad_shapes():
    from gtsfm_amd import native

    q = native.lib().gtsfm_patchmatchnet_workspace_bytes
    assert q(3, 2, 72, 104) > 0
    for n, s, h, w in ((0, 2, 72, 104), (-1, 2, 72, 104), (3, 0, 72, 104), (3, 2, 0, 104), (3, 2, 72, -8),
                       (3, 2, 70, 104), (3, 2, 72, 100)):
        assert q(n, s, h, w) == 0


def test_missing_checkpoint_is_a_clear_error(tmp_path):
    from gtsfm_amd.densify import MVSPatchmatchNet

    with pytest.raises(FileNotFoundError, match="checkpoint not found"):
        MVSPatchmatchNet(str(tmp_path / "model_000007.ckpt"))
