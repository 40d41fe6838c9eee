"""gtsfm_d2net_batched and the D2NetDetDesc plugin on the GPU against the fp64 torch restatement (tests/d2net_ref.py,
itself pinned to the reference by tests/test_d2net_ref.py).

The dense map is held to the PatchmatchNet rule: the kernel's error against the fp64 run (median and 99th percentile,
relative to the map's maximum) may be at most 4 x the error of the restatement's own fp32 run. A detection is a
discrete decision, so keypoints are compared only where fp32 cannot flip it: elements within a slack (100 x the fp32
map error) of any threshold are left out, and over the rest the detected set must be the restatement's exactly.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import d2net_ref as dref  # noqa: E402
from d2net_weights import d2net_state_dict, textured_image  # noqa: E402

pytestmark = pytest.mark.gpu

ALL = 2048  # a max_keypoints above every candidate count here


@pytest.fixture(scope="module")
def sd():
    return d2net_state_dict(0)


@pytest.fixture(scope="module")
def blob(sd):
    from gtsfm_amd.frontend.detector_descriptor.d2net import pack_d2net_weights

    return torch.from_numpy(pack_d2net_weights(sd)).cuda()


@pytest.fixture(scope="module")
def images():
    """small: 48 x 64 -> an 11 x 15 map, one partial tile, the dilated halo outside the map on every side;
    large: 100 x 140 -> 24 x 34, more than one 32-column and more than one 16-row tile."""
    with np.load(os.path.join(HERE, "golden", "d2net_random_w0.npz")) as z:
        return {"small": z["a__image"], "large": textured_image(1, 100, 140), "gray": z["b__image"]}


@pytest.fixture(scope="module")
def truth(sd, images):
    """Per image the restatement's fp64 and fp32 runs, computed once and left unchanged."""
    return {k: (dref.run(sd, images[k], torch.float64), dref.run(sd, images[k], torch.float32))
            for k in ("small", "large")}


def _extract(blob, imgs, k, dense=False, out=None):
    from gtsfm_amd import device

    t = torch.from_numpy(np.ascontiguousarray(np.stack(imgs))).cuda()
    res = device.d2net_extract(t, blob, k, dense_map=dense, out=out)
    torch.cuda.synchronize()
    return res


def _np(res):
    return {f: getattr(res, f).cpu().numpy() for f in ("xy", "scores", "desc", "count", "n_candidates")}


@pytest.fixture(scope="module")
def full(blob, images):
    """One call per image with the dense map and every candidate kept."""
    out = {}
    for k in ("small", "large"):
        res = _extract(blob, [images[k]], ALL, dense=True)
        d = _np(res)
        d["dense"] = res.dense_map.cpu().numpy()[0].transpose(2, 0, 1)  # (512, h, w)
        out[k] = d
    return out


@pytest.mark.parametrize("name", ("small", "large"))
def test_dense_map(full, truth, name):
    r64, r32 = truth[name]
    got = full[name]["dense"]
    assert got.shape == r64["dense"].shape
    k_med, k_p99, k_max = dref.map_error(got, r64["dense"])
    y_med, y_p99, y_max = dref.map_error(r32["dense"], r64["dense"])
    print(f"{name}: map {got.shape} max {r64['dense'].max():.4g}; kernel error median {k_med:.3g} p99 {k_p99:.3g} max "
          f"{k_max:.3g}; fp32 restatement median {y_med:.3g} p99 {y_p99:.3g} max {y_max:.3g}")
    assert k_med <= 4 * y_med
    assert k_p99 <= 4 * y_p99


def _gpu_candidates(g):
    """(c, i, j) of the call's keypoints: the location is the rounded map position (|step| < 0.5), the channel the one
    whose map value is the score."""
    n = int(g["count"][0])
    ij = np.round((g["xy"][0, :n, ::-1].astype(np.float64) - 1.5) / 4).astype(np.int64)
    c = g["dense"][:, ij[:, 0], ij[:, 1]].argmax(0)
    assert np.array_equal(g["dense"][c, ij[:, 0], ij[:, 1]], g["scores"][0, :n]), "a score is not its map value"
    return np.concatenate([c[:, None], ij], axis=1)


@pytest.mark.parametrize("name", ("small", "large"))
def test_keypoints(full, truth, name):
    r64, r32 = truth[name]
    g = full[name]
    n = int(g["count"][0])
    assert n == int(g["n_candidates"][0]) > 50
    slack = dref.slack_for(r32["dense"], r64["dense"])
    cij = _gpu_candidates(g)
    missing, spurious, dropped = dref.compare_detected(dref.margins(r64["dense"]), slack, cij)
    print(f"{name}: {n} keypoints, restatement {len(r64['cij'])}; slack {slack:.3g}; dropped share {dropped:.4f}; "
          f"missing {len(missing)} spurious {len(spurious)}")
    assert dropped < 0.05
    assert len(missing) == 0 and len(spurious) == 0
    assert np.all(np.diff(g["scores"][0, :n]) <= 0), "not in descending score"
    # matched keypoints
    key64 = {tuple(t): q for q, t in enumerate(r64["cij"].tolist())}
    pairs = [(q, key64[tuple(t)]) for q, t in enumerate(cij.tolist()) if tuple(t) in key64]
    assert len(pairs) >= 0.95 * len(r64["cij"])
    qg, qr = np.array(pairs).T
    up = r64["cand_pos"][qr][:, ::-1] * 4 + 1.5
    dxy = np.abs(g["xy"][0, qg] - up).max()
    score_bound = 4 * dref.map_error(r32["dense"], r64["dense"])[2] * r64["dense"].max()
    dscore = np.abs(g["scores"][0, qg] - r64["cand_score"][qr]).max()
    ddesc = np.abs(g["desc"][0, qg] - r64["cand_desc"][qr]).max()
    print(f"{name}: {len(pairs)} matched: xy {dxy:.3g} px, score {dscore:.3g} (bound {score_bound:.3g}), "
          f"descriptor {ddesc:.3g}")
    assert dxy <= 1e-3
    assert dscore <= score_bound
    assert ddesc <= 1e-5
    np.testing.assert_allclose(np.linalg.norm(g["desc"][0, :n], axis=1), 1.0, atol=1e-5)


def test_topk_cut(blob, images, full):
    from gtsfm_amd import device

    g = full["small"]
    n = int(g["count"][0])
    cut = _np(_extract(blob, [images["small"]], 32))
    assert cut["count"][0] == 32 and cut["n_candidates"][0] == n > 32
    for f in ("xy", "scores", "desc"):
        assert np.array_equal(cut[f][0], g[f][0, :32]), f
    # more room than candidates: count == candidates, and the rows past it are zeroed, not left as they were
    dev = blob.device
    out = device.D2NetResult(torch.full((1, ALL, 2), np.nan, device=dev), torch.full((1, ALL), np.nan, device=dev),
                             torch.full((1, ALL, 512), np.nan, device=dev),
                             torch.full((1,), -1, dtype=torch.int32, device=dev),
                             torch.full((1,), -1, dtype=torch.int32, device=dev))
    big = _np(_extract(blob, [images["small"]], ALL, out=out))
    assert big["count"][0] == big["n_candidates"][0] == n
    for f in ("xy", "scores", "desc"):
        assert np.array_equal(big[f][0, :n], g[f][0, :n]), f
        assert not np.any(big[f][0, n:]), f"{f}: rows past the count are not zero"


def test_batch_equals_single_calls_and_repeats(blob):
    imgs = [textured_image(s, 48, 64) for s in (2, 3, 4)]
    batch = _np(_extract(blob, imgs, 200))
    again = _np(_extract(blob, imgs, 200))
    for f in batch:
        assert batch[f].tobytes() == again[f].tobytes(), f"{f}: two identical calls differ"
    assert len(set(batch["count"].tolist())) > 1 or len(set(batch["scores"][:, 0].tolist())) == 3
    for i, im in enumerate(imgs):
        one = _np(_extract(blob, [im], 200))
        for f in batch:
            assert batch[f][i].tobytes() == one[f][0].tobytes(), f"image {i} {f}: batch and single call differ"


def test_plugin(tmp_path, sd, blob, images):
    from gtsfm_amd.common.image import Image
    from gtsfm_amd.frontend.detector_descriptor import D2NetDetDesc

    path = tmp_path / "d2_tf.pth"
    torch.save({"model": {k: torch.from_numpy(v) for k, v in sd.items()}}, str(path))
    det = D2NetDetDesc(max_keypoints=60, model_path=path)
    for name in ("small", "gray"):
        im = images[name]
        assert im.ndim == (2 if name == "gray" else 3)
        kp, desc = det.detect_and_describe(Image(im))
        want = _np(_extract(blob, [dref.to_rgb(im)], 60))
        n = int(want["count"][0])
        assert n == 60 and desc.shape == (n, 512) and desc.dtype == np.float32
        assert np.array_equal(kp.coordinates, want["xy"][0, :n])
        assert np.array_equal(kp.responses, want["scores"][0, :n])
        assert np.array_equal(desc, want["desc"][0, :n])
        np.testing.assert_allclose(np.linalg.norm(desc, axis=1), 1.0, atol=1e-5)
        x, y = kp.coordinates[:, 0], kp.coordinates[:, 1]
        assert x.min() >= 0 and x.max() < im.shape[1] and y.min() >= 0 and y.max() < im.shape[0]
    res = det.detect_and_describe_batch_device([Image(images["small"]), Image(textured_image(3, 48, 64))])
    assert res.xy.is_cuda and res.desc.shape == (2, 60, 512)
    assert np.array_equal(res.xy[0].cpu().numpy(), _np(_extract(blob, [images["small"]], 60))["xy"][0])


def test_plugin_oversize_image_comes_back_in_its_own_frame(tmp_path, sd):
    """Over MAX_EDGE_PX: an 8 x 1700 strip of noise, reflect-padded to 40 columns (8 columns are below the smallest
    image the network takes), is resized to 1600 x 37 on the device; coordinates come back in the 1700 x 40 frame."""
    from gtsfm_amd.common.image import Image
    from gtsfm_amd.frontend.detector_descriptor import D2NetDetDesc
    from gtsfm_amd.frontend.detector_descriptor.d2net import resized_shape

    strip = np.random.default_rng(5).integers(0, 256, (1700, 8, 3), dtype=np.uint8)
    im = np.pad(strip, ((0, 0), (16, 16), (0, 0)), mode="reflect")
    H, W = im.shape[:2]
    assert resized_shape(H, W)[:2] == (1600, 37)
    det = D2NetDetDesc(max_keypoints=500, state_dict=sd)
    kp, desc = det.detect_and_describe(Image(im))
    assert len(kp.coordinates) > 100 and desc.shape == (len(kp.coordinates), 512)
    x, y = kp.coordinates[:, 0], kp.coordinates[:, 1]
    assert x.min() >= 0 and x.max() < W and y.min() >= 0 and y.max() < H
    assert y.max() > 1600, "the rows were not scaled back to the original frame"


def test_argument_checks_touch_no_output(blob):
    from gtsfm_amd import native

    L = native.lib()
    dev = blob.device
    k, H, W = 16, 48, 64
    img = torch.zeros((1, H, W, 3), dtype=torch.uint8, device=dev)
    need = L.gtsfm_d2net_workspace_bytes(1, H, W, k)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    xy, sc = torch.full((1, k, 2), 7.0, device=dev), torch.full((1, k), 7.0, device=dev)
    de = torch.full((1, k, 512), 7.0, device=dev)
    cnt = torch.full((1,), 7, dtype=torch.int32, device=dev)
    s = native.stream_handle(None)

    def call(H=H, k=k, xy_ptr=xy.data_ptr(), ws_bytes=need, w_ptr=blob.data_ptr()):
        return L.gtsfm_d2net_batched(img.data_ptr(), 1, H, W, 3, w_ptr, k, 1.0, 1.0, ws.data_ptr(), ws_bytes, xy_ptr,
                                     sc.data_ptr(), de.data_ptr(), cnt.data_ptr(), None, None, s)

    assert call(H=8) == native.GTSFM_ERR_ARG
    assert call(xy_ptr=None) == native.GTSFM_ERR_ARG
    assert call(w_ptr=None) == native.GTSFM_ERR_ARG
    assert call(k=0) == native.GTSFM_ERR_ARG
    assert call(k=-3) == native.GTSFM_ERR_ARG
    assert call(ws_bytes=need - 1) == native.GTSFM_ERR_CAPACITY
    torch.cuda.synchronize()
    assert bool((xy == 7).all()) and bool((sc == 7).all()) and bool((de == 7).all()) and int(cnt[0]) == 7
    assert call() == native.GTSFM_OK
    torch.cuda.synchronize()
    assert 0 <= int(cnt[0]) <= k and not bool((de == 7).any())
