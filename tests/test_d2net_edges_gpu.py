"""gtsfm_d2net_batched at the edges that tests/test_d2net_gpu.py cannot see, compared exactly.

Same-map detection: the call returns its dense map, and the restatement's detect / describe (tests/d2net_ref.py) run
in float32 on the CPU on that very map. Both sides then evaluate the same IEEE float32 expressions in the same order,
so the candidate list, its order, the scores and the positions must be identical, with no slack and nothing left out
(tests/test_d2net_planted.py checks that the float32 restatement is a sound oracle). Only the descriptors get 1e-6:
the kernel sums the squared norm with an FMA, and that is all the room a unit vector needs.

Planted maps (tests/d2net_planted.py): pass-through weights under which the map is an exactly known function of a
block image. They hold the trunk's indexing (tile seams, partial tiles, the dilated halo, the fused max-pools, the
eight output-channel tiles) to bit equality, and they plant exact channel ties, a candidate list that overflows and an
image without candidates. The preconditions of every case are asserted without a GPU in tests/test_d2net_planted.py.
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
from d2net_weights import d2net_state_dict, textured_image  # noqa: E402

pytestmark = pytest.mark.gpu

SRC = dp.channel_sources()
FIELDS = ("xy", "scores", "desc", "count", "n_candidates")


def _blob(sd):
    from gtsfm_amd.frontend.detector_descriptor.d2net import pack_d2net_weights

    return torch.from_numpy(pack_d2net_weights(sd)).cuda()


@pytest.fixture(scope="module")
def sd():
    return d2net_state_dict(0)


@pytest.fixture(scope="module")
def blob(sd):
    return _blob(sd)


@pytest.fixture(scope="module")
def tie_blob():
    return _blob(dp.passthrough_state_dict(SRC, dp.tie_gains()))


@pytest.fixture(scope="module")
def images():
    """small, large: those of tests/test_d2net_gpu.py. 75x139: H and W odd, H / 2 = 37 and W / 2 = 69 odd, a 17 x 33
    map, one row and one column past a tile edge (the seed is one with corner rejections). 12x200: a 2 x 49 strip,
    every location on a border row. 12x12: the smallest legal image, a 2 x 2 map."""
    with np.load(os.path.join(HERE, "golden", "d2net_random_w0.npz")) as z:
        small = z["a__image"]
    return {"small": small, "large": textured_image(1, 100, 140), "75x139": textured_image(10, 75, 139),
            "12x200": textured_image(7, 12, 200), "12x12": textured_image(8, 12, 12)}


def _call(blob, imgs, k, fact_i=1.0, fact_j=1.0, guard=False):
    """One call on the images as a batch, with the dense map. guard: the outputs are the leading slices of NaN-filled
    buffers one image larger (counts -1), so rows past a count must be written (zeroed) and nothing past the last
    image's row k - 1 may be. Returns numpy arrays; dense is (n, 512, h, w)."""
    from gtsfm_amd import device

    n = len(imgs)
    t = torch.from_numpy(np.ascontiguousarray(np.stack(imgs))).cuda()
    out = buf = None
    if guard:
        dev = t.device
        buf = device.D2NetResult(torch.full((n + 1, k, 2), np.nan, device=dev),
                                 torch.full((n + 1, k), np.nan, device=dev),
                                 torch.full((n + 1, k, 512), np.nan, device=dev),
                                 torch.full((n + 1,), -1, dtype=torch.int32, device=dev),
                                 torch.full((n + 1,), -1, dtype=torch.int32, device=dev))
        out = device.D2NetResult(buf.xy[:n], buf.scores[:n], buf.desc[:n], buf.count[:n], buf.n_candidates[:n])
    res = device.d2net_extract(t, blob, k, fact_i=fact_i, fact_j=fact_j, out=out, dense_map=True)
    torch.cuda.synchronize()
    if guard:
        for f in ("xy", "scores", "desc"):
            assert bool(torch.isnan(getattr(buf, f)[n]).all()), f"{f}: written past the last row"
        assert int(buf.count[n]) == -1 and int(buf.n_candidates[n]) == -1
    g = {f: getattr(res, f).cpu().numpy() for f in FIELDS}
    g["dense"] = np.ascontiguousarray(res.dense_map.cpu().numpy().transpose(0, 3, 1, 2))
    return g


def _one(g, i=0):
    return {f: g[f][i] for f in g}


def _expected(dense, k, fact_i=1.0, fact_j=1.0):
    """The restatement in float32 on the map `dense` (512, h, w): what the call must return for it. The per-image
    list holds h w candidates: of more, the first h w in (i, j, c) order are kept, then listed in (c, i, j) order."""
    h, w = dense.shape[1:]
    Fm = torch.from_numpy(dense)
    with torch.no_grad():
        det = dref.detect(Fm)
        n_all = len(det["cij"])
        keep = dp.overflow_kept(det["cij"], h * w) if n_all > h * w else np.arange(n_all)
        cij, pi, pj, score = det["cij"][keep], det["pi"][keep], det["pj"][keep], det["score"][keep]
        assert pi.dtype == pj.dtype == score.dtype == np.float32
        order = np.argsort(-score, kind="stable")[:k]
        desc = dref.describe(Fm, pi[order], pj[order])
    xy = np.stack([pj[order], pi[order]], axis=1)
    for _ in range(2):
        xy = xy * np.float32(2.0) + np.float32(0.5)
    xy = xy * np.array([fact_j, fact_i], np.float32)
    assert xy.dtype == np.float32
    return dict(n_all=n_all, n_kept=len(keep), cij=cij[order], xy=xy, scores=score[order], desc=desc,
                all_cij=det["cij"], all_score=det["score"], full_order=np.argsort(-score, kind="stable"),
                rejected=(det["rejected_edge"], det["rejected_step"], det["rejected_corner"]))


def _listed_cij(g, fact_i, fact_j):
    """(c, i, j) of the call's rows, from its outputs alone: the location is the rounded map position (|step| < 0.5);
    the channels whose map value is the score are dealt out in ascending order to the rows of one location and score
    (rows of an exact tie are identical in every output, and the candidate order lists the lower channel first)."""
    n = int(g["count"])
    pos = g["xy"][:n, ::-1].astype(np.float64) / np.array([fact_i, fact_j])
    ij = np.round((pos - 1.5) / 4).astype(np.int64)
    seen, out = {}, []
    for (i, j), s in zip(ij.tolist(), g["scores"][:n].tolist()):
        cs = np.flatnonzero(g["dense"][:, i, j] == np.float32(s))
        q = seen.get((i, j, s), 0)
        assert q < len(cs), f"row at ({i}, {j}) with score {s}: more rows than channels with that map value"
        out.append((int(cs[q]), i, j))
        seen[(i, j, s)] = q + 1
    return np.array(out, np.int64).reshape(-1, 3)


def _check_same_map(g, k, fact_i=1.0, fact_j=1.0, label=""):
    """g: one image's outputs of a call with max_keypoints k. Returns the expectation for further checks."""
    e = _expected(g["dense"], k, fact_i, fact_j)
    n = min(e["n_kept"], k)
    print(f"{label}: map {g['dense'].shape[1:]}, {e['n_all']} candidates ({e['n_kept']} held), k {k}, count "
          f"{int(g['count'])}; rejected edge / step / corner {e['rejected']}")
    assert int(g["n_candidates"]) == e["n_all"]
    assert int(g["count"]) == n
    assert g["scores"][:n].tobytes() == e["scores"].tobytes(), "scores or their order differ"
    assert np.all(np.diff(g["scores"][:n]) <= 0)
    cij = _listed_cij(g, fact_i, fact_j)
    assert np.array_equal(cij, e["cij"]), "the (c, i, j) list or its order differs"
    assert np.array_equal(g["dense"][cij[:, 0], cij[:, 1], cij[:, 2]], g["scores"][:n]), "a score is not its map value"
    bad = np.flatnonzero((g["xy"][:n] != e["xy"]).any(axis=1))
    assert len(bad) == 0, (f"{len(bad)} positions differ, first row {bad[0]}: {g['xy'][bad[0]]} against "
                           f"{e['xy'][bad[0]]} at (c, i, j) {cij[bad[0]]}")
    if n:
        ddesc = float(np.abs(g["desc"][:n] - e["desc"]).max())
        print(f"{label}: descriptor difference {ddesc:.3g}")
        assert ddesc <= 1e-6
    for f in ("xy", "scores", "desc"):
        assert not np.any(g[f][n:]), f"{f}: rows past the count are not zero"
    return e


# ------------------------------------------------------------------ 1. same-map exactness, random weights
@pytest.mark.parametrize("name,fact", (("small", (1.0, 1.0)), ("large", (1.0, 1.0)), ("75x139", (1.0, 1.0)),
                                       ("12x200", (1.0, 1.0)), ("75x139", (1.0625, 0.9375))))
def test_same_map_detection_is_exact(blob, images, name, fact):
    g = _one(_call(blob, [images[name]], 2048, fact[0], fact[1], guard=True))
    e = _check_same_map(g, 2048, fact[0], fact[1], label=f"{name} fact {fact}")
    assert e["n_all"] >= (10 if name == "12x200" else 50)


def test_edge_ratio_exactly_on_the_threshold_is_kept():
    """tr^2 / det == 7.2f exactly (tests/d2net_planted.edge_threshold_case): `<=` keeps the one detection."""
    sd_edge, img, want = dp.edge_threshold_case()
    g = _one(_call(_blob(sd_edge), [img], 8, guard=True))
    assert g["dense"].tobytes() == want.tobytes()
    e = _check_same_map(g, 8, label="edge threshold")
    assert e["n_all"] == 1 and e["cij"].tolist() == [[dp.EDGE_CHANNEL, 3, 3]]
    assert g["xy"][0].tolist() == [13.5, 13.5] and g["scores"][0] == 12.0


# ------------------------------------------------------------------ 2. exact planted maps at tile seams
@pytest.fixture(scope="module")
def seam_blob():
    return _blob(dp.passthrough_state_dict(SRC, dp.seam_gains()))


@pytest.mark.parametrize("name", sorted(dp.SEAM_CASES))
def test_planted_map_is_exact_at_tile_seams(seam_blob, name):
    H4, W4, er, ec = dp.SEAM_CASES[name]
    u = dp.noise_blocks(7, H4, W4)
    got = _call(seam_blob, [dp.block_image(u, er, ec)], 16)["dense"][0]
    want = dp.planted_map(u, SRC, dp.seam_gains())
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (f"{len(bad)} of {want.size} map values differ, first (c, i, j) {bad[0]}: "
                           f"{got[tuple(bad[0])]} against {want[tuple(bad[0])]}")
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("name", sorted(dp.SHIFT_CASES))
def test_shifted_tap_is_exact_across_seams_and_border(name):
    layer, tap = dp.SHIFT_CASES[name]
    sd_shift = dp.passthrough_state_dict(SRC, dp.seam_gains(), taps={layer: tap})
    img = dp.block_image(dp.noise_blocks(7, *dp.SHIFT_GRID))
    with torch.no_grad():
        want = dref.dense_map(sd_shift, img, torch.float32).numpy()
    got = _call(_blob(sd_shift), [img], 16)["dense"][0]
    assert got.shape == want.shape == (512, 17, 33)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (f"{len(bad)} of {want.size} map values differ, first (c, i, j) {bad[0]}: "
                           f"{got[tuple(bad[0])]} against {want[tuple(bad[0])]}")
    assert got.tobytes() == want.tobytes()


# ------------------------------------------------------------------ 3. ties
def _tie_run(blob, gain, k, guard=True):
    u = dp.case_blocks(dp.TIE_CASE)
    g = _one(_call(blob, [dp.block_image(u)], k, guard=guard))
    assert g["dense"].tobytes() == dp.planted_map(u, SRC, gain).tobytes()
    return g


def _check_cut(blob, gain, full, e, k):
    """The call with max_keypoints k keeps exactly the first k rows of the full result."""
    assert e["scores"][k - 1] == e["scores"][k], "the cut is not inside a tie"
    cut = _tie_run(blob, gain, k)
    assert int(cut["count"]) == k and int(cut["n_candidates"]) == e["n_all"]
    for f in ("xy", "scores", "desc"):
        assert cut[f].tobytes() == full[f][:k].tobytes(), f"{f}: not the first {k} rows of the full result"


def test_two_way_ties(tie_blob):
    gain = dp.tie_gains()
    full = _tie_run(tie_blob, gain, 512)
    e = _check_same_map(full, 512, label="two-way ties")
    pairs = dp.tied_groups(e["all_score"], e["all_cij"])
    assert e["n_all"] > 256 and len(pairs) >= 50
    k = dp.cut_between_blocks(e["all_score"], e["full_order"], pairs)
    assert k is not None
    a, b = e["full_order"][k - 1], e["full_order"][k]
    print(f"two-way ties: {len(pairs)} tied pairs; cut k = {k} between candidates {a} and {b} of {e['n_all']}, "
          f"channels {e['all_cij'][a, 0]} and {e['all_cij'][b, 0]}")
    assert a // 256 != b // 256
    _check_cut(tie_blob, gain, full, e, k)


def test_three_way_ties():
    gain = dp.tie_gains(three_way=True)
    blob3 = _blob(dp.passthrough_state_dict(SRC, gain))
    full = _tie_run(blob3, gain, 512)
    e = _check_same_map(full, 512, label="three-way ties")
    triples = [t for t in dp.tied_groups(e["all_score"], e["all_cij"]) if len(t) == 3]
    assert len(triples) >= 20
    k1 = dp.cut_between_blocks(e["all_score"], e["full_order"], triples, member=1)
    k2 = dp.cut_between_blocks(e["all_score"], e["full_order"], triples, member=2)
    print(f"three-way ties: {len(triples)} triples; cuts after the first member k = {k1}, after the second k = {k2}")
    assert k1 is not None and k2 is not None
    _check_cut(blob3, gain, full, e, k1)
    _check_cut(blob3, gain, full, e, k2)


# ------------------------------------------------------------------ 4. list overflow
@pytest.mark.parametrize("k", (600, 100))
def test_candidate_list_overflow(k):
    gain = np.ones(512, np.float32)
    u = dp.case_blocks(dp.OVERFLOW_CASE)
    g = _one(_call(_blob(dp.passthrough_state_dict(SRC, gain)), [dp.block_image(u)], k, guard=True))
    assert g["dense"].tobytes() == dp.planted_map(u, SRC, gain).tobytes()
    e = _check_same_map(g, k, label=f"overflow k {k}")
    assert e["n_all"] > 561 == e["n_kept"]
    assert int(g["count"]) == min(561, k) and int(g["n_candidates"]) == e["n_all"]


# ------------------------------------------------------------------ 5. zero candidates and mixed batches
def test_black_image_and_mixed_batch(tie_blob):
    k = 256
    black = np.zeros((72, 136, 3), np.uint8)
    planted = [dp.block_image(dp.noise_blocks(s, 18, 34)) for s in (2, 3)]
    singles = [_call(tie_blob, [im], k, guard=True) for im in (planted[0], black, planted[1])]
    b = singles[1]
    assert int(b["count"][0]) == 0 and int(b["n_candidates"][0]) == 0 and not b["dense"].any()
    for f in ("xy", "scores", "desc"):
        assert not np.any(b[f]), f"{f}: rows of an image without candidates are not zero"
    batch = _call(tie_blob, [planted[0], black, planted[1]], k, guard=True)
    counts = batch["count"].tolist()
    print(f"mixed batch: counts {counts}, candidates {batch['n_candidates'].tolist()}")
    assert counts[1] == 0 and 50 < counts[0] < k and 50 < counts[2] < k and counts[0] != counts[2]
    for i, one in enumerate(singles):
        for f in FIELDS + ("dense",):
            assert batch[f][i].tobytes() == one[f][0].tobytes(), f"image {i} {f}: batch and single call differ"
    for i in (0, 2):
        _check_same_map(_one(batch, i), k, label=f"mixed batch image {i}")


# ------------------------------------------------------------------ 6. dense map at the new shapes against fp64
@pytest.mark.parametrize("name", ("75x139", "12x200", "12x12"))
def test_dense_map_at_new_shapes(sd, blob, images, name):
    with torch.no_grad():
        d64 = dref.dense_map(sd, images[name], torch.float64).numpy()
        d32 = dref.dense_map(sd, images[name], torch.float32).numpy()
    got = _call(blob, [images[name]], 64)["dense"][0]
    assert got.shape == d64.shape == (512,) + tuple(t // 4 - 1 for t in images[name].shape[:2])
    k_med, k_p99, k_max = dref.map_error(got, d64)
    y_med, y_p99, y_max = dref.map_error(d32, d64)
    print(f"{name}: map {got.shape} max {d64.max():.4g}; kernel error median {k_med:.3g} p99 {k_p99:.3g} max "
          f"{k_max:.3g}; fp32 restatement median {y_med:.3g} p99 {y_p99:.3g} max {y_max:.3g}")
    assert k_med <= 4 * y_med
    if name == "12x12" and y_p99 == 0:
        assert k_max <= 4 * y_max
    else:
        assert k_p99 <= 4 * y_p99
