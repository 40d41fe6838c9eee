"""The planted-map helper (tests/d2net_planted.py) without a GPU: its closed form against the restatement's float32
map bit for bit, the preconditions that tests/test_d2net_edges_gpu.py relies on (ties, list overflow, no candidates,
nonzero seams), and the restatement's handling of exact channel ties against a case recorded from the reference's own
detection and localisation modules (tests/golden/d2net_planted_ties.npz, made by tests/golden/make_d2net_golden.py)."""
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
from d2net_weights import d2net_state_dict, textured_image  # noqa: E402

SRC = dp.channel_sources()


def _ref_map(sd, img):
    with torch.no_grad():
        return dref.dense_map(sd, img, torch.float32).numpy()


def _detect(Fm):
    with torch.no_grad():
        return dref.detect(torch.from_numpy(Fm))


@pytest.mark.parametrize("name", sorted(dp.SEAM_CASES))
@pytest.mark.parametrize("gains", ("seam", "tie"))
def test_planted_map_is_the_restatements_fp32_map(name, gains):
    H4, W4, er, ec = dp.SEAM_CASES[name]
    u = dp.noise_blocks(7, H4, W4)
    gain = dp.seam_gains() if gains == "seam" else dp.tie_gains()
    img = dp.block_image(u, er, ec)
    assert img.shape == (4 * H4 + er, 4 * W4 + ec, 3)
    want = dp.planted_map(u, SRC, gain)
    got = _ref_map(dp.passthrough_state_dict(SRC, gain), img)
    assert want.shape == got.shape == (512, H4 - 1, W4 - 1) == (512,) + tuple(int(t) for t in name.split("x"))
    assert want.tobytes() == got.tobytes()
    assert np.isfinite(want).all() and (want[want > 0] >= np.finfo(np.float32).tiny).all()


def test_planted_map_with_a_last_layer_bias():
    u = dp.noise_blocks(8, 5, 9)
    bias = np.linspace(-0.5, 0.5, 512).astype(np.float32)
    got = _ref_map(dp.passthrough_state_dict(SRC, dp.tie_gains(), bias=bias), dp.block_image(u, 1, 2))
    assert got.tobytes() == dp.planted_map(u, SRC, dp.tie_gains(), bias=bias).tobytes()


def test_seam_gains_tell_every_channel_apart():
    g = dp.seam_gains()
    assert len({(int(s), float(v)) for s, v in zip(SRC, g)}) == 512
    m, e = np.frexp(g)
    assert np.all(m == 0.5) and e.min() == -84 and e.max() == 86  # 2 ** -85 .. 2 ** 85


@pytest.mark.parametrize("name", sorted(dp.SEAM_CASES))
def test_seam_maps_are_nonzero_on_both_sides_of_each_seam(name):
    """Tiles are 16 rows x 32 columns: the last row / column of a tile and the first of the next (or the map's last)
    carry a nonzero value of every source, so a wrong read there cannot hide behind a zero."""
    H4, W4, _, _ = dp.SEAM_CASES[name]
    G = dp.planted_source(dp.noise_blocks(7, H4, W4))
    h, w = G.shape[1:]
    for c in range(3):
        for r in {min(15, h - 1), min(16, h - 1), 0, h - 1}:
            assert G[c, r].any(), (c, r)
        for q in {min(31, w - 1), min(32, w - 1), 0, w - 1}:
            assert G[c, :, q].any(), (c, q)


def _shifted(a, di, dj):
    """out[..., y, x] = a[..., y + di, x + dj], zero outside."""
    out = np.zeros_like(a)
    h, w = a.shape[-2:]
    ys, xs = slice(max(0, -di), min(h, h - di)), slice(max(0, -dj), min(w, w - dj))
    yd, xd = slice(max(0, di), min(h, h + di)), slice(max(0, dj), min(w, w + dj))
    out[..., ys, xs] = a[..., yd, xd]
    return out


@pytest.mark.parametrize("name", sorted(dp.SHIFT_CASES))
def test_shift_cases_move_values_across_the_seams(name):
    layer, (ky, kx) = dp.SHIFT_CASES[name]
    u = dp.noise_blocks(7, *dp.SHIFT_GRID)
    gain = dp.seam_gains()
    plain = dp.planted_map(u, SRC, gain)
    got = _ref_map(dp.passthrough_state_dict(SRC, gain, taps={layer: (ky, kx)}), dp.block_image(u))
    assert got.shape == plain.shape == (512, 17, 33)
    assert (got != plain).mean() > 0.5
    if layer >= 7:  # a dilated layer acts on the map itself: a shift by 2 (k - 1), zero filled
        assert got.tobytes() == _shifted(plain, 2 * (ky - 1), 2 * (kx - 1)).tobytes()
    for c in range(3):  # nonzero on both sides of the seams at row 15 | 16 and column 31 | 32
        assert all(got[c, r].any() for r in (15, 16) if 0 <= r + 2 * (ky - 1) < 17)
        assert all(got[c, :, q].any() for q in (31, 32) if 0 <= q + 2 * (kx - 1) < 33)


def _tie_stats(three_way):
    u = dp.case_blocks(dp.TIE_CASE)
    det = _detect(dp.planted_map(u, SRC, dp.tie_gains(three_way)))
    order = np.argsort(-det["score"], kind="stable")
    return det, order, dp.tied_groups(det["score"], det["cij"])


def test_tie_case_preconditions():
    det, order, groups = _tie_stats(False)
    n = len(det["cij"])
    pairs = [g for g in groups if len(g) == 2]
    k = dp.cut_between_blocks(det["score"], order, pairs)
    print(f"tie case: {n} candidates in channels {sorted(set(det['cij'][:, 0].tolist()))}, {len(pairs)} tied pairs, "
          f"rejected edge / step / corner {det['rejected_edge']} / {det['rejected_step']} / {det['rejected_corner']}, "
          f"cut k = {k}")
    assert n > 256
    assert len(pairs) >= 50 and len(pairs) == len(groups)
    assert set(det["cij"][:, 0].tolist()) == set(dp.TIE_CHANNELS)
    assert det["rejected_edge"] >= 1 and det["rejected_step"] >= 1
    # both members of a pair are listed, the lower channel first, with one position
    for a, b in pairs:
        assert det["cij"][b, 0] - det["cij"][a, 0] == 300
        assert det["pi"][a] == det["pi"][b] and det["pj"][a] == det["pj"][b]
    assert k is not None and 0 < k < n
    assert det["score"][order[k - 1]] == det["score"][order[k]] and order[k - 1] // 256 != order[k] // 256


def test_three_way_tie_case_preconditions():
    det, order, groups = _tie_stats(True)
    triples = [g for g in groups if len(g) == 3]
    k1 = dp.cut_between_blocks(det["score"], order, triples, member=1)
    k2 = dp.cut_between_blocks(det["score"], order, triples, member=2)
    print(f"three-way tie case: {len(det['cij'])} candidates, {len(triples)} triples, {len(groups) - len(triples)} "
          f"pairs, cuts k = {k1}, {k2}")
    assert len(det["cij"]) > 256 and len(triples) >= 20
    for g in triples:
        assert det["cij"][g, 0].tolist() == [0, dp.THIRD_COPY, 300]
    assert k1 is not None and k2 is not None
    for k in (k1, k2):
        assert det["score"][order[k - 1]] == det["score"][order[k]]


def test_overflow_case_preconditions():
    u = dp.case_blocks(dp.OVERFLOW_CASE)
    det = _detect(dp.planted_map(u, SRC, np.ones(512, np.float32)))
    h, w = dp.OVERFLOW_CASE["H4"] - 1, dp.OVERFLOW_CASE["W4"] - 1
    n = len(det["cij"])
    print(f"overflow case: {n} candidates, list capacity {h * w}")
    assert (h, w) == (17, 33) and n > 561 == h * w
    kept = dp.overflow_kept(det["cij"], h * w)
    assert len(kept) == h * w and np.all(np.diff(kept) > 0)
    # the cut falls inside a location's run of channels, and the kept set spans many channels
    last = det["cij"][kept][:, 1:].max(axis=0)
    ij = det["cij"][:, 1] * w + det["cij"][:, 2]
    cut = np.sort(ij)[h * w - 1]
    assert 0 < (ij[kept] == cut).sum() < (ij == cut).sum(), "the capacity does not cut a location's channels apart"
    assert len(set(det["cij"][kept][:, 0].tolist())) > 100 and last[0] < h - 1


def test_black_image_has_no_candidates():
    img = dp.block_image(np.zeros((18, 34, 3), np.uint8))
    Fm = _ref_map(dp.passthrough_state_dict(SRC, dp.tie_gains()), img)
    assert Fm.shape == (512, 17, 33) and not Fm.any()
    assert len(_detect(Fm)["cij"]) == 0


def test_edge_threshold_case_sits_exactly_on_the_threshold():
    sd, img, want = dp.edge_threshold_case()
    Fm = _ref_map(sd, img)
    assert Fm.tobytes() == want.tobytes()
    c = dp.EDGE_CHANNEL
    assert Fm[c, 2:5, 2:5].tolist() == [[6, 7, 6], [11, 12, 11], [6, 7, 6]]
    with torch.no_grad():
        q = dref.fields(torch.from_numpy(Fm))
    assert float(q["det"][c, 3, 3]) == 20 and float(q["tr"][c, 3, 3]) == -12
    assert q["ratio"].dtype == torch.float32 and float(q["ratio"][c, 3, 3]) == float(np.float32(7.2))
    det = _detect(Fm)
    assert det["cij"].tolist() == [[c, 3, 3]] and det["pi"].tolist() == [3.0] and det["pj"].tolist() == [3.0]
    # the ridges' ends: the zero padding makes them detections with a step of exactly 0.5, which |step| < 0.5 rejects
    assert det["rejected_step"] == 4 and det["rejected_edge"] == 0 and det["rejected_corner"] == 0
    assert sorted({abs(float(q[k][c, i, j])) for k, i, j in (("step_j", 3, 0), ("step_j", 3, 6), ("step_i", 0, 3),
                                                             ("step_i", 6, 3))}) == [0.5]


def test_fp32_restatement_detects_what_fp64_does_on_one_map():
    """What the same-map GPU test rests on: on one float32 map the float32 and the float64 evaluation of the
    detection agree on the candidate list, so the float32 restatement is a sound oracle for the kernel."""
    Fm = _ref_map(d2net_state_dict(0), textured_image(1, 100, 140))
    d32 = _detect(Fm)
    d64 = _detect(Fm.astype(np.float64))
    assert len(d32["cij"]) > 500
    assert np.array_equal(d32["cij"], d64["cij"])
    assert np.abs(d32["pi"] - d64["pi"]).max() < 1e-3 and np.abs(d32["pj"] - d64["pj"]).max() < 1e-3


def test_odd_image_of_the_same_map_test_has_every_rejection():
    """The 75 x 139 image of tests/test_d2net_edges_gpu.py: the edge, step and corner tests each reject something."""
    det = _detect(_ref_map(d2net_state_dict(0), textured_image(10, 75, 139)))
    assert len(det["cij"]) > 300
    assert det["rejected_edge"] >= 1 and det["rejected_step"] >= 1 and det["rejected_corner"] >= 1


def test_restatement_ties_equal_the_reference():
    """Exact channel ties: both tied channels are candidates, in torch.nonzero order, in the reference's own modules
    as in the restatement."""
    with np.load(os.path.join(HERE, "golden", "d2net_planted_ties.npz")) as z:
        g = {k: z[k] for k in z.files}
    sd = dp.passthrough_state_dict(SRC, dp.tie_gains())
    r = dref.run(sd, g["image"], torch.float32)
    assert g["image"].nbytes > 0 and len(g["cij"]) > 100
    assert np.array_equal(r["cij"], g["cij"])
    assert r["cand_score"].dtype == np.float32 and np.array_equal(r["cand_score"], g["scores"])
    pairs = dp.tied_groups(g["scores"], g["cij"])
    assert len(pairs) >= 20 and all(g["cij"][b, 0] - g["cij"][a, 0] == 300 for a, b in pairs)
    # the reference sums its 3 x 3 derivative filters in its own order: positions agree to fp32 rounding
    pos = (r["cand_pos"] * 2 + 0.5) * 2 + 0.5
    np.testing.assert_allclose(pos, g["kp"], rtol=0, atol=1e-3)
    # and the restatement in fp64 on the same (exact) map lists the same candidates
    assert np.array_equal(dref.run(sd, g["image"], torch.float64)["cij"], g["cij"])
