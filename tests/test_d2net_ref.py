"""D2-Net without a GPU: the torch restatement (tests/d2net_ref.py) against outputs recorded from the reference's own
modules (tests/golden/d2net_random_w0.npz, made by tests/golden/make_d2net_golden.py), the golden's non-degeneracy,
the weight blob's layout, the workspace query and the plugin's resize rule."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import d2net_ref as dref  # noqa: E402
from d2net_weights import D2NET_LAYERS, PREFIX, d2net_state_dict  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "d2net_random_w0.npz")
CASES = ("a", "b")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def runs(golden):
    sd = d2net_state_dict(0)
    return {c: dref.run(sd, golden[f"{c}__image"], torch.float64) for c in CASES}


def _upscaled(pos):
    for _ in range(2):
        pos = pos * 2 + 0.5
    return pos


@pytest.mark.parametrize("case", CASES)
def test_restatement_equals_reference_fp64(golden, runs, case):
    r = runs[case]
    # the golden map is the reference's fp64 map stored as fp32: narrowed the same way, the restatement's is the same
    got, want = r["dense"].astype(np.float32), golden[f"{case}__dense"]
    assert got.shape == want.shape
    assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 1e-10
    kp, scores = golden[f"{case}__kp_f64"], golden[f"{case}__scores_f64"]
    # the candidate set and its order: process_multiscale lists (i, j) upscaled, in torch.nonzero's order
    assert len(r["cij"]) == len(kp)
    np.testing.assert_array_equal(np.round((kp - 1.5) / 4).astype(np.int64), r["cij"][:, 1:])
    np.testing.assert_allclose(_upscaled(r["cand_pos"]), kp, rtol=0, atol=1e-9)
    np.testing.assert_allclose(r["cand_score"], scores, rtol=0, atol=1e-10)
    assert np.all(np.lexsort((r["cij"][:, 2], r["cij"][:, 1], r["cij"][:, 0])) == np.arange(len(kp)))
    rows = golden[f"{case}__desc_rows"]
    np.testing.assert_allclose(r["cand_desc"][rows], golden[f"{case}__desc_f64"], rtol=0, atol=1e-9)
    # the final keypoints: descending score, (x, y)
    assert np.all(np.diff(r["scores"]) <= 0)
    np.testing.assert_allclose(r["xy"], kp[r["order"]][:, ::-1], rtol=0, atol=1e-9)


@pytest.mark.parametrize("case", CASES)
def test_restatement_fp32_close_to_reference_fp32(golden, case):
    r = dref.run(d2net_state_dict(0), golden[f"{case}__image"], torch.float32)
    kp = golden[f"{case}__kp_f32"]
    assert len(r["cij"]) == len(kp)
    np.testing.assert_allclose(_upscaled(r["cand_pos"]), kp, rtol=0, atol=1e-3)
    np.testing.assert_allclose(r["cand_desc"][golden[f"{case}__desc_rows"]], golden[f"{case}__desc_f32"], rtol=0,
                               atol=1e-5)


@pytest.mark.parametrize("case", CASES)
def test_golden_is_not_degenerate(golden, runs, case):
    r = runs[case]
    assert len(golden[f"{case}__scores_f64"]) >= 50
    assert r["rejected_edge"] >= 1 and r["rejected_step"] >= 1 and r["rejected_corner"] >= 1
    positive = float((golden[f"{case}__dense"] > 0).mean())
    assert 0.05 < positive < 0.95, "the seeded weights give an all-zero or saturated map"
    assert golden[f"{case}__image"].std() > 20, "the image is (nearly) constant"


@pytest.mark.parametrize("name", ("a", "large"))
def test_gpu_test_images_are_decidable(golden, name):
    """The condition tests/test_d2net_gpu.py puts on its inputs, checked with the restatement's fp32 run standing in
    for the kernel: under 5 % of the candidates lie within the slack of a threshold, and away from the thresholds the
    fp32 run detects exactly what the fp64 run does."""
    from d2net_weights import textured_image

    sd = d2net_state_dict(0)
    image = golden["a__image"] if name == "a" else textured_image(1, 100, 140)
    r64, r32 = dref.run(sd, image, torch.float64), dref.run(sd, image, torch.float32)
    slack = dref.slack_for(r32["dense"], r64["dense"])
    missing, spurious, dropped = dref.compare_detected(dref.margins(r64["dense"]), slack, r32["cij"])
    print(f"{name}: fp32 map error (median, p99, max) {dref.map_error(r32['dense'], r64['dense'])}, slack {slack:.3g}, "
          f"dropped share {dropped:.4f} of {len(r64['cij'])} candidates")
    assert dropped < 0.05
    assert len(missing) == 0 and len(spurious) == 0


def test_d2net_weight_blob_layout():
    from gtsfm_amd.frontend.detector_descriptor.d2net import pack_d2net_weights

    sd = d2net_state_dict(3)
    blob = pack_d2net_weights(sd)
    assert blob.dtype == np.float32
    assert blob.size == sum(9 * cin * cout + cout for _, cin, cout in D2NET_LAYERS) == 7635264
    o = 0
    for idx, cin, cout in D2NET_LAYERS:
        w, b = sd[f"{PREFIX}.{idx}.weight"], sd[f"{PREFIX}.{idx}.bias"]
        W = blob[o:o + 9 * cin * cout].reshape(9, cin, cout)
        for ky, kx, ci, co in ((0, 0, 0, 0), (1, 2, cin - 1, 5), (2, 1, cin // 2, cout - 1)):
            assert W[ky * 3 + kx, ci, co] == w[co, ci, ky, kx]
        o += 9 * cin * cout
        np.testing.assert_array_equal(blob[o:o + cout], b)
        o += cout
    assert o == blob.size


def test_d2net_workspace_query_needs_no_gpu():
    from gtsfm_amd import native

    L = native.lib()
    assert L.gtsfm_d2net_weights_floats() == 7635264
    small, large = L.gtsfm_d2net_workspace_bytes(1, 48, 64, 32), L.gtsfm_d2net_workspace_bytes(3, 100, 140, 500)
    assert 0 < small < large
    for shape in ((0, 48, 64, 32), (1, 0, 0, 32), (1, 8, 64, 32), (1, 48, 11, 32), (1, 48, 64, 0)):
        assert L.gtsfm_d2net_workspace_bytes(*shape) == 0, shape


def test_d2net_resize_rule():
    from gtsfm_amd.frontend.detector_descriptor.d2net import MAX_EDGE_PX, MAX_SUM_EDGES_PX, resized_shape

    H, W = 1080, 1920
    s1 = MAX_EDGE_PX / max(H, W)
    h1, w1 = int(H * s1), int(W * s1)
    assert h1 + w1 <= MAX_SUM_EDGES_PX  # 900 + 1600: the second limit does not bite
    assert resized_shape(H, W) == (h1, w1, H / h1, W / w1) == (900, 1600, 1.2, 1.2)
    assert resized_shape(600, 800) == (600, 800, 1.0, 1.0)
    # both limits: 1500 x 1590 passes the first and trips the second
    s2 = MAX_SUM_EDGES_PX / (1500 + 1590)
    assert resized_shape(1500, 1590) == (int(1500 * s2), int(1590 * s2), 1500 / int(1500 * s2), 1590 / int(1590 * s2))


def test_d2net_plugin_construction_and_pickle(tmp_path):
    import pickle

    from gtsfm_amd.frontend.detector_descriptor import D2NetDetDesc
    from gtsfm_amd.frontend.detector_descriptor.detector_descriptor_base import DetectorDescriptorBase

    with pytest.raises(FileNotFoundError, match="D2-Net checkpoint not found"):
        D2NetDetDesc(model_path=tmp_path / "missing.pth")
    path = tmp_path / "d2_tf.pth"
    torch.save({"model": {k: torch.from_numpy(v) for k, v in d2net_state_dict(0).items()}}, str(path))
    det = D2NetDetDesc(max_keypoints=77, model_path=path)
    assert isinstance(det, DetectorDescriptorBase)
    det._blob = object()  # stands in for the device copy
    clone = pickle.loads(pickle.dumps(det))
    assert type(clone) is D2NetDetDesc and clone.max_keypoints == 77 and clone._blob is None
    np.testing.assert_array_equal(clone._packed, det._packed)
