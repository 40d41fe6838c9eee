"""gtsfm_patchmatchnet_batched on the MI355X where tests/test_patchmatchnet_gpu.py does not look: every view of every
case as the reference view against the fp64 restatement (tests/patchmatchnet_ref.py, tied to the reference's module by
tests/test_patchmatchnet_ref.py), with a maximum and not only a median; the smallest accepted shape, (c); maps of more
than one 16 x 16 tile on every level, (d); ragged source rows; a view without a source; the workspace's earlier
contents; a side stream. Cases (c) and (d): tests/patchmatchnet_cases.py.

Bounds. Depths (the five iteration depths and the refined depth), per view, against fp64: median and 99th percentile at
most 4 x the fp32 restatement's own on the same pixels, and no pixel beyond 1e-4 of the view's depth range
(tests/test_patchmatchnet_ref.py holds the fp32 restatement alone to a quarter of that on (c) and (d), the golden
records the same for (a) and (b)). Confidence, on pixels whose fp64 regression index is more than 1e-3 from an integer
(the truncated index is a switch): the same median and 99th percentile, and the largest error at most 4 x the fp32
restatement's largest. Feature maps: 2e-4 of the map's largest value.

Measured on the MI355X: see DESIGN.md, "PatchmatchNet".
"""
import os

import numpy as np
import pytest
import torch

import patchmatchnet_cases as pcases
import patchmatchnet_ref as pref
from patchmatchnet_weights import patchmatchnet_state_dict
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = ("a", "b", "c", "d")
DEPTHS = ["iter0", "iter1", "iter2", "iter3", "iter4", "depth"]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def cases():
    with np.load(os.path.join(GOLDEN, "patchmatchnet_random_w0.npz")) as z:
        out = {name: pref.load_golden_case(z, name) for name in ("a", "b")}
    out.update(pcases.cases())
    return out


@pytest.fixture(scope="module")
def state_dict():
    return patchmatchnet_state_dict(0)


@pytest.fixture(scope="module")
def blob(state_dict):
    from gtsfm_amd.densify import pack_patchmatchnet_weights

    return _t(pack_patchmatchnet_weights(state_dict))


@pytest.fixture(scope="module")
def expected(cases, state_dict):
    """{case: [per view (fp32 outputs, fp64 outputs)]} of the restatement on the CPU, computed once."""
    return {name: [tuple(pcases.restatement(state_dict, case, v, dtype) for dtype in (torch.float32, torch.float64))
                   for v in range(case["images"].shape[0])] for name, case in cases.items()}


@pytest.fixture(scope="module")
def expected_features(cases, state_dict):
    """{case: {stage: (n, h, w, C) float64}}: FeatureNet of every view in fp64."""
    sd = pref.torch_state_dict(state_dict, torch.float64)
    out = {}
    for name, case in cases.items():
        img = torch.from_numpy(case["images"].astype(np.float64) / 255.0).permute(0, 3, 1, 2)
        with torch.no_grad():
            out[name] = {s: f.permute(0, 2, 3, 1).numpy() for s, f in pref.feature_net(sd, img).items()}
    return out


def _run(case, blob, views=None, uniform=None, src_views=None, workspace=None, stream=None):
    from gtsfm_amd import device

    views = list(range(case["images"].shape[0])) if views is None else views
    uniform = pref.batch_uniform(case)[views] if uniform is None else uniform
    src_views = case["src_views"][views] if src_views is None else np.asarray(src_views)
    r = device.patchmatchnet_depth(_t(case["images"][views]), _t(case["wRc"][views]), _t(case["wtc"][views]),
                                   _t(case["intrinsics"][views]), _t(src_views.astype(np.int32)),
                                   _t(case["depth_range"][views]), blob, _t(uniform), debug=True, workspace=workspace,
                                   stream=stream)
    torch.cuda.synchronize()
    return r


def _outputs(r):
    """Every output of a call as one list of tensors: depth, confidence, the three feature maps, the five depths."""
    return [r.depth, r.confidence, *r.features, *r.iter_depths]


def _equal(a, b, view_a=None, view_b=None):
    """Bit for bit (NaN equal to NaN), the whole batch or one view of each."""
    return all(torch.equal((x if view_a is None else x[view_a]).view(torch.int32),
                           (y if view_b is None else y[view_b]).view(torch.int32))
               for x, y in zip(_outputs(a), _outputs(b)))


@pytest.fixture(scope="module")
def batched(cases, blob):
    """Every view of each case as a reference view, in one call per case."""
    return {name: _run(cases[name], blob) for name in CASES}


def _view_outputs(r, v):
    got = {f"iter{i}": d[v].cpu().numpy() for i, d in enumerate(r.iter_depths)}
    got.update(depth=r.depth[v].cpu().numpy(), confidence=r.confidence[v].cpu().numpy())
    return got


def _away(index):
    """Full-resolution mask of the pixels whose stage-1 regression index is more than 1e-3 from an integer."""
    return np.repeat(np.repeat(np.abs(index - np.round(index)) > 1e-3, 2, 0), 2, 1)


def _spans(case):
    return case["depth_range"][:, 1] - case["depth_range"][:, 0]


@pytest.mark.parametrize("name", CASES)
def test_every_view_depths_against_fp64(cases, expected, batched, name):
    case, r = cases[name], batched[name]
    n = case["images"].shape[0]
    assert r.depth.shape == case["images"].shape[:3] and r.confidence.shape == r.depth.shape
    failures = []
    for v in range(n):
        got, (r32, r64), span = _view_outputs(r, v), expected[name][v], float(_spans(case)[v])
        for key in DEPTHS:
            assert got[key].shape == r64[key].shape, (v, key)
            assert np.isfinite(got[key]).all(), (v, key)
            ref = pref.error_figures(r32[key], r64[key], span)
            mine = pref.error_figures(got[key], r64[key], span)
            ref_max = np.abs(r32[key].astype(np.float64) - r64[key]).max() / span
            mine_max = np.abs(got[key].astype(np.float64) - r64[key]).max() / span
            print(f"case {name} view {v} {key}: kernel median {mine[0]:.3g} p99 {mine[1]:.3g} max/range {mine_max:.3g}"
                  f" | restatement fp32 median {ref[0]:.3g} p99 {ref[1]:.3g} max/range {ref_max:.3g}")
            if not (mine[0] <= 4 * ref[0] and mine[1] <= 4 * ref[1] and mine_max <= 1e-4):
                failures.append((v, key))
    assert not failures, failures


@pytest.mark.parametrize("name", CASES)
def test_every_view_confidence_against_fp64(cases, expected, batched, name):
    case, r = cases[name], batched[name]
    failures = []
    for v in range(case["images"].shape[0]):
        got, (r32, r64) = r.confidence[v].cpu().numpy(), expected[name][v]
        assert np.isfinite(got).all(), v
        keep = _away(r64["index"])
        want = r64["confidence"][keep]
        ref = pref.error_figures(r32["confidence"][keep], want, 1.0)
        mine = pref.error_figures(got[keep], want, 1.0)
        ref_max = np.abs(r32["confidence"][keep].astype(np.float64) - want).max()
        mine_max = np.abs(got[keep].astype(np.float64) - want).max()
        print(f"case {name} view {v} confidence: kernel median {mine[0]:.3g} p99 {mine[1]:.3g} max {mine_max:.3g} | "
              f"restatement fp32 median {ref[0]:.3g} p99 {ref[1]:.3g} max {ref_max:.3g}")
        if not (mine[0] <= 4 * ref[0] and mine[1] <= 4 * ref[1] and mine_max <= 4 * ref_max):
            failures.append(v)
    assert not failures, failures


@pytest.mark.parametrize("name", CASES)
def test_every_view_features_against_fp64(cases, expected_features, batched, name):
    """All three maps of every view (they feed every warp): 2e-4 of the map's largest value, the tolerance the project
    uses for fp32 networks with another summation order."""
    for got, stage in zip(batched[name].features, (3, 2, 1)):
        want = expected_features[name][stage]
        assert tuple(got.shape) == want.shape
        for v in range(want.shape[0]):
            err = np.abs(got[v].cpu().numpy() - want[v]).max() / np.abs(want[v]).max()
            print(f"case {name} view {v} stage {stage} feature error / max {err:.3g}")
            assert err <= 2e-4, (v, stage)


def _regions(h, w):
    """The ring of border pixels; rows or columns 15, 16 and 17 (the first tile seam) off the ring; the rest."""
    ys, xs = np.mgrid[0:h, 0:w]
    ring = (ys == 0) | (ys == h - 1) | (xs == 0) | (xs == w - 1)
    seam = ((ys >= 15) & (ys <= 17) | (xs >= 15) & (xs <= 17)) & ~ring
    return {"ring": ring, "seam": seam, "rest": ~ring & ~seam}


@pytest.mark.parametrize("name", CASES)
def test_locality_report(cases, expected, expected_features, batched, name):
    """Where the largest error of each output lies: a failure of the bounds above then says whether it is a border, a
    tile seam or neither. Asserts the bounds of the tests above and nothing else."""
    case, r = cases[name], batched[name]
    for v in range(case["images"].shape[0]):
        got, (_, r64), span = _view_outputs(r, v), expected[name][v], float(_spans(case)[v])
        keep = _away(r64["index"])
        for key in DEPTHS + ["confidence"]:
            err = np.abs(got[key].astype(np.float64) - r64[key]) / (1.0 if key == "confidence" else span)
            if key == "confidence":
                err = np.where(keep, err, 0.0)
            figures = {k: (float(err[m].max()) if m.any() else 0.0) for k, m in _regions(*err.shape).items()}
            print(f"case {name} view {v} {key}: largest error " + " ".join(f"{k} {e:.3g}" for k, e in figures.items()))
            if key != "confidence":
                assert max(figures.values()) <= 1e-4, (v, key)
        for feat, stage in zip(r.features, (3, 2, 1)):
            want = expected_features[name][stage][v]
            err = np.abs(feat[v].cpu().numpy() - want).max(axis=2) / np.abs(want).max()
            figures = {k: (float(err[m].max()) if m.any() else 0.0) for k, m in _regions(*err.shape).items()}
            print(f"case {name} view {v} feature {stage}: largest error / max " +
                  " ".join(f"{k} {e:.3g}" for k, e in figures.items()))
            assert max(figures.values()) <= 2e-4, (v, stage)


def test_ragged_row_equals_compact_row(cases, blob, batched):
    """(d): the view whose row is [-1, 0, 2] gets, bit for bit, the result of a call that holds only that view and its
    valid sources as a full n_src = 2 row."""
    case, r = cases["d"], batched["d"]
    v = 1
    assert list(case["src_views"][v]) == [-1, 0, 2]
    views = [v] + pcases.valid_sources(case, v)
    rows = [[1, 2], [0, 2], [0, 1]]
    alone = _run(case, blob, views=views, src_views=rows)
    assert alone.depth.shape[0] == 3
    assert _equal(alone, r, 0, v)
    # and the other ragged rows: trailing -1, an index >= n
    for v in (0, 2):
        views = [v] + pcases.valid_sources(case, v)
        assert _equal(_run(case, blob, views=views, src_views=rows), r, 0, v), v


def test_every_invalid_index_is_the_same(cases, blob, batched):
    """-1, an index >= n, n itself and the smallest int in the same slots: the same bits."""
    case, n = cases["d"], 3
    for a, b in ((7, -1), (n, 2 ** 31 - 1), (-(2 ** 31), -2)):
        rows = [[1, 2, a], [b, 0, 2], [a, 1, 0]]
        assert _equal(_run(case, blob, src_views=rows), batched["d"]), (a, b)


def test_a_changed_row_changes_only_its_view(cases, blob, batched):
    case, r = cases["d"], batched["d"]
    changed = _run(case, blob, src_views=[[2, -1, -1], [-1, 0, 2], [7, 1, 0]])  # view 0 loses source 1
    assert _equal(changed, r, 1, 1) and _equal(changed, r, 2, 2)
    assert not torch.equal(changed.depth[0], r.depth[0]), "the changed row was not read"
    # the same source twice: the restatement with that source twice, and again no other view moves
    twice = _run(case, blob, src_views=[[1, 2, -1], [-1, 0, 2], [1, 7, 1]])
    assert _equal(twice, r, 0, 0) and _equal(twice, r, 1, 1)
    assert not torch.equal(twice.depth[2], r.depth[2])


def test_a_source_named_twice_against_fp64(cases, state_dict, blob):
    """View 2 of (d) with source 1 in two slots around an invalid one: the restatement with the sources [1, 1]."""
    case = cases["d"]
    r = _run(case, blob, src_views=[[1, 2, -1], [-1, 0, 2], [1, 7, 1]])
    one = dict(case, src_views=np.array([[1, 2, -1], [-1, 0, 2], [1, 7, 1]], np.int32))
    r32, r64 = (pcases.restatement(state_dict, one, 2, dtype) for dtype in (torch.float32, torch.float64))
    got, span = _view_outputs(r, 2), float(_spans(case)[2])
    for key in DEPTHS:
        ref, mine = pref.error_figures(r32[key], r64[key], span), pref.error_figures(got[key], r64[key], span)
        mine_max = np.abs(got[key].astype(np.float64) - r64[key]).max() / span
        print(f"{key}: kernel median {mine[0]:.3g} p99 {mine[1]:.3g} max/range {mine_max:.3g} | restatement fp32 "
              f"median {ref[0]:.3g} p99 {ref[1]:.3g}")
        assert mine[0] <= 4 * ref[0] and mine[1] <= 4 * ref[1] and mine_max <= 1e-4, key


def test_a_view_without_a_source(cases, blob, batched):
    """The other views are bit for bit those of the call where that view has sources. The view itself has no matching
    cost (0 / 0 in the weighted mean over the sources); the header promises that its confidence passes no `> threshold`
    test."""
    case, r = cases["d"], batched["d"]
    none = _run(case, blob, src_views=[[1, 2, -1], [-1, 7, -1], [7, 1, 0]])
    assert _equal(none, r, 0, 0) and _equal(none, r, 2, 2)
    conf, depth = none.confidence[1], none.depth[1]
    print(f"view without a source: confidence finite {int(torch.isfinite(conf).sum())} of {conf.numel()}, largest "
          f"finite {float(torch.nan_to_num(conf, nan=0.0).max()):.3g}; depth finite {int(torch.isfinite(depth).sum())}")
    assert not bool((conf > 0).any())
    # the features of that view do not depend on its row
    for a, b in zip(none.features, r.features):
        assert torch.equal(a, b)


def test_result_does_not_depend_on_the_workspace(cases, blob, batched):
    """(d) with the default workspace, with a caller's larger workspace full of 0xFF bytes (NaN), and with a workspace
    that has just served case (a), of another shape: the same bits."""
    from gtsfm_amd import native

    case, r = cases["d"], batched["d"]
    n, H, W = case["images"].shape[:3]
    need = int(native.lib().gtsfm_patchmatchnet_workspace_bytes(n, case["src_views"].shape[1], H, W))
    ws = torch.full((need + 4096,), 0xFF, dtype=torch.uint8, device=DEV)
    assert _equal(_run(case, blob, workspace=ws), r)
    assert not bool((ws[:need] == 0xFF).all()), "the caller's workspace was not used"
    assert bool((ws[need:] == 0xFF).all()), "written past the queried size"
    a = _run(cases["a"], blob, workspace=ws)
    assert _equal(a, batched["a"])
    assert _equal(_run(case, blob, workspace=ws), r)


def test_short_workspace_is_refused_and_touches_nothing(cases, blob):
    from gtsfm_amd import native

    L = native.lib()
    case = cases["c"]
    n, H, W = case["images"].shape[:3]
    S = case["src_views"].shape[1]
    need = int(L.gtsfm_patchmatchnet_workspace_bytes(n, S, H, W))
    ins = [_t(case["images"]), _t(case["wRc"]), _t(case["wtc"]), _t(case["intrinsics"]), _t(case["src_views"]),
           _t(case["depth_range"]), _t(pref.batch_uniform(case))]
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device=DEV)
    depth, conf = (torch.full((n, H, W), 7.0, device=DEV) for _ in range(2))
    feat = torch.full((n * (H // 8 * (W // 8) * 64 + H // 4 * (W // 4) * 32 + H // 2 * (W // 2) * 16),), 7.0, device=DEV)
    iters = torch.full((n * (2 * (H // 8) * (W // 8) + 2 * (H // 4) * (W // 4) + (H // 2) * (W // 2)),), 7.0, device=DEV)

    def call(ws_bytes):
        rc = L.gtsfm_patchmatchnet_batched(ins[0].data_ptr(), n, H, W, ins[1].data_ptr(), ins[2].data_ptr(),
                                           ins[3].data_ptr(), ins[4].data_ptr(), S, ins[5].data_ptr(), blob.data_ptr(),
                                           ins[6].data_ptr(), None, ws.data_ptr(), ws_bytes, depth.data_ptr(),
                                           conf.data_ptr(), feat.data_ptr(), iters.data_ptr(),
                                           native.stream_handle(None))
        torch.cuda.synchronize()
        return rc

    assert call(need - 1) == native.GTSFM_ERR_CAPACITY
    assert all(bool((t == 7).all()) for t in (depth, conf, feat, iters)) and bool((ws == 0x5A).all())
    assert call(need) == native.GTSFM_OK
    assert not any(bool((t == 7).any()) for t in (depth, conf, feat, iters))


def test_side_stream_equals_default_stream(cases, blob, batched):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        r = _run(cases["c"], blob, stream=side)
    side.synchronize()
    assert _equal(r, batched["c"])
