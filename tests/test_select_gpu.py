"""The top-k selection rule that SuperPoint and D2-Net share (gtsfm_amd/csrc/select.hpp), through the two public entry
points: of N candidates the k highest scores are kept, and of those equal to the k-th score the earliest in candidate
order.

Both halves state the selection given the scores, not the networks: the expectation is computed in numpy from the
scores and positions of a call that keeps everything, and compared bit for bit.
- SuperPoint keeps its selection in raster order (the candidate order): max_kpts = N, N - 1 and 1 on the smallest golden
  image.
- D2-Net ranks its selection by descending score, equal scores in candidate order: the planted three-way-tie map of
  tests/d2net_planted.py (its preconditions: tests/test_d2net_planted.py), cut one, two and three rows into a triple of
  exactly equal scores. tests/test_d2net_edges_gpu.py::test_three_way_ties checks the same map against the
  restatement with the cuts placed between 256-candidate blocks; here the three cuts walk through one triple.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import d2net_planted as dp  # noqa: E402
import d2net_ref as dref  # noqa: E402
from superpoint_weights import superpoint_state_dict  # noqa: E402

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ SuperPoint: kept in raster order
@pytest.fixture(scope="module")
def sp_full(golden_dir):
    """(detector, image, N, xy, scores, desc) of the 240 x 320 golden image with max_kpts above the detection count."""
    from gtsfm_amd import native
    from gtsfm_amd.frontend.detector_descriptor.superpoint import SuperPointDetectorDescriptor

    native.require_gpu()
    det = SuperPointDetectorDescriptor(max_keypoints=16384, state_dict=superpoint_state_dict(0))
    with np.load(os.path.join(golden_dir, "superpoint_random_w0.npz")) as z:
        img = z["synthetic_240x320__image"]
    res = det.extract_batch([img])
    n = int(res.count[0])
    assert n == int(res.n_detected[0]) and n > 256  # more than one 256-candidate block
    xy = res.xy[0, :n].cpu().numpy()
    assert np.array_equal(np.lexsort((xy[:, 0], xy[:, 1])), np.arange(n)), "the full result is not in raster order"
    return det, img, n, xy, res.scores[0, :n].cpu().numpy(), res.desc[0, :n].cpu().numpy()


@pytest.mark.parametrize("drop", ("none", "one", "all_but_one"))
def test_superpoint_keeps_the_k_highest_in_raster_order(sp_full, drop):
    det, img, n, xy, sc, desc = sp_full
    k = {"none": n, "one": n - 1, "all_but_one": 1}[drop]
    # the k highest scores, equal scores to the earliest raster position (stable sort), listed in raster order
    keep = np.sort(np.argsort(-sc, kind="stable")[:k])
    res = det.extract_batch([img], max_kpts=k)
    assert int(res.count[0]) == k and int(res.n_detected[0]) == n
    assert res.xy[0].cpu().numpy().tobytes() == xy[keep].tobytes()
    assert res.scores[0].cpu().numpy().tobytes() == sc[keep].tobytes()
    assert res.desc[0].cpu().numpy().tobytes() == desc[keep].tobytes()


# ------------------------------------------------------------------ D2-Net: ranked, ties in candidate order
def _d2_call(blob, img, k):
    from gtsfm_amd import device

    res = device.d2net_extract(torch.from_numpy(img[None]).cuda(), blob, k, dense_map=True)
    torch.cuda.synchronize()
    out = {f: getattr(res, f)[0].cpu().numpy() for f in ("xy", "scores", "desc", "count", "n_candidates")}
    out["dense"] = np.ascontiguousarray(res.dense_map[0].cpu().numpy().transpose(2, 0, 1))
    return out


@pytest.fixture(scope="module")
def d2_tie():
    """The three-way-tie map: (blob, image, full call, candidate scores and (x, y) in ranked order, first row of a
    triple of equal scores)."""
    from gtsfm_amd.frontend.detector_descriptor.d2net import pack_d2net_weights

    gain = dp.tie_gains(three_way=True)
    src = dp.channel_sources()
    u = dp.case_blocks(dp.TIE_CASE)
    img = dp.block_image(u)
    blob = torch.from_numpy(pack_d2net_weights(dp.passthrough_state_dict(src, gain))).cuda()
    full = _d2_call(blob, img, 512)
    want_map = dp.planted_map(u, src, gain)
    assert full["dense"].tobytes() == want_map.tobytes()
    with torch.no_grad():
        det = dref.detect(torch.from_numpy(want_map))
    n = len(det["cij"])
    assert n <= 512 and n <= want_map.shape[1] * want_map.shape[2], "the candidate list overflows: not this test's case"
    order = np.argsort(-det["score"], kind="stable")  # descending score, equal scores in candidate (c, i, j) order
    xy = np.stack([det["pj"][order], det["pi"][order]], axis=1)
    for _ in range(2):
        xy = xy * np.float32(2.0) + np.float32(0.5)
    assert xy.dtype == np.float32
    score = det["score"][order]
    triples = [g for g in dp.tied_groups(det["score"], det["cij"]) if len(g) == 3]
    row_of = np.empty(n, np.int64)
    row_of[order] = np.arange(n)
    g = triples[0]
    r = int(row_of[g[0]])
    assert row_of[g].tolist() == [r, r + 1, r + 2] and det["cij"][g, 0].tolist() == [0, dp.THIRD_COPY, 300]
    assert score[r] == score[r + 2] and (r == 0 or score[r - 1] > score[r]) and score[r + 3] < score[r]
    # the full call is the restatement's ranking
    assert int(full["count"]) == n == int(full["n_candidates"])
    assert full["scores"][:n].tobytes() == score.tobytes() and full["xy"][:n].tobytes() == xy.tobytes()
    return blob, img, full, score, xy, r


@pytest.mark.parametrize("members", (1, 2, 3))
def test_d2net_cut_inside_a_three_way_tie(d2_tie, members):
    blob, img, full, score, xy, r = d2_tie
    k = r + members
    got = _d2_call(blob, img, k)
    assert int(got["count"]) == k and int(got["n_candidates"]) == len(score)
    assert got["scores"].tobytes() == score[:k].tobytes()
    assert got["xy"].tobytes() == xy[:k].tobytes()
    assert got["desc"].tobytes() == full["desc"][:k].tobytes()
