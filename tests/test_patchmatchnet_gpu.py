"""gtsfm_patchmatchnet_batched on the MI355X against the reference's recorded outputs
(tests/golden/patchmatchnet_random_w0.npz, made by tests/golden/make_patchmatchnet_golden.py).

No error bar is fixed in advance: the fp32 reference's own error against its fp64 run is measured from the golden on
the same pixels (median, 99th percentile, share of pixels above 1e-4 of the depth range) and the kernels, compared with
the same fp64 outputs, may have at most 4 x that median and 99th percentile (another summation order through about
twenty chained layers) and at most 1 % of pixels more above 1e-4 of the range.

Measured on the MI355X (kernel | reference fp32, both against the reference's fp64): see DESIGN.md, "PatchmatchNet".
"""
import os

import numpy as np
import pytest
import torch

import patchmatchnet_ref as pref
from patchmatchnet_weights import patchmatchnet_state_dict
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = ("a", "b")
OUTPUTS = ["iter0", "iter1", "iter2", "iter3", "iter4", "depth", "confidence"]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "patchmatchnet_random_w0.npz")) as z:
        return {name: pref.load_golden_case(z, name) for name in CASES}


@pytest.fixture(scope="module")
def blob():
    from gtsfm_amd.densify import pack_patchmatchnet_weights

    return _t(pack_patchmatchnet_weights(patchmatchnet_state_dict(0)))


def _run(case, blob, views=None, uniform=None, src_views=None, config=None):
    from gtsfm_amd import device

    views = list(range(case["images"].shape[0])) if views is None else views
    uniform = pref.batch_uniform(case)[views] if uniform is None else uniform
    src_views = case["src_views"][views] if src_views is None else src_views
    r = device.patchmatchnet_depth(_t(case["images"][views]), _t(case["wRc"][views]), _t(case["wtc"][views]),
                                   _t(case["intrinsics"][views]), _t(src_views.astype(np.int32)),
                                   _t(case["depth_range"][views]), blob, _t(uniform), debug=True, config=config)
    torch.cuda.synchronize()
    return r


@pytest.fixture(scope="module")
def batched(golden, blob):
    """Every view of each case as a reference view, in one call per case."""
    return {name: _run(golden[name], blob) for name in CASES}


@pytest.mark.parametrize("name", CASES)
def test_feature_maps(golden, batched, name):
    """The tolerance the project uses for fp32 networks with another summation order (SuperPoint's descriptors): 2e-4
    of the map's largest value."""
    for got, stage in zip(batched[name].features, (3, 2, 1)):
        want = golden[name][f"feat{stage}"]
        err = np.abs(got[0].permute(2, 0, 1).cpu().numpy() - want).max() / np.abs(want).max()
        print(f"case {name} stage {stage} feature error / max {err:.3g}")
        assert err <= 2e-4


@pytest.mark.parametrize("name", CASES)
def test_depths_and_confidence_against_fp64(golden, batched, name):
    case, r = golden[name], batched[name]
    assert r.depth.shape == case["images"].shape[:3] and r.confidence.shape == r.depth.shape
    got = {f"iter{i}": d[0].cpu().numpy() for i, d in enumerate(r.iter_depths)}
    got.update(depth=r.depth[0].cpu().numpy(), confidence=r.confidence[0].cpu().numpy())
    span = float(case["depth_range"][0, 1] - case["depth_range"][0, 0])
    index = case["index_f64"]
    away = np.abs(index - np.round(index)) > 1e-3  # the truncated index is a switch: compared where it is not near one
    away = np.repeat(np.repeat(away, 2, 0), 2, 1)
    failures = []
    for key in OUTPUTS:
        assert np.isfinite(got[key]).all(), key
        keep = away if key == "confidence" else np.ones(got[key].shape, bool)
        s = 1.0 if key == "confidence" else span
        ref = pref.error_figures(case[f"{key}_f32"][keep], case[f"{key}_f64"][keep], s)
        mine = pref.error_figures(got[key][keep], case[f"{key}_f64"][keep], s)
        print(f"case {name} {key}: kernel median {mine[0]:.3g} p99 {mine[1]:.3g} share {mine[2]:.4f} | reference fp32 "
              f"median {ref[0]:.3g} p99 {ref[1]:.3g} share {ref[2]:.4f}")
        if not (mine[0] <= 4 * ref[0] and mine[1] <= 4 * ref[1] and mine[2] <= ref[2] + 0.01):
            failures.append(key)
    assert not failures, failures


def test_batch_equals_each_view_alone(golden, blob, batched):
    """Case (b): a view's result in the batch of five is bit for bit the result of a call that holds only that view and
    its sources: the features are shared, and nothing leaks from one reference view to the next."""
    case, r = golden["b"], batched["b"]
    uniform = pref.batch_uniform(case)
    for v in range(case["images"].shape[0]):
        views = [v] + [int(s) for s in case["src_views"][v]]
        rows = np.array([[j for j in range(len(views)) if j != i] for i in range(len(views))], np.int32)
        alone = _run(case, blob, views=views, uniform=uniform[views], src_views=rows)
        assert torch.equal(alone.depth[0], r.depth[v]) and torch.equal(alone.confidence[0], r.confidence[v]), v
        for a, b in zip(alone.iter_depths, r.iter_depths):
            assert torch.equal(a[0], b[v]), v


@pytest.mark.parametrize("name", CASES)
def test_two_runs_are_bit_identical(golden, blob, batched, name):
    again = _run(golden[name], blob)
    assert torch.equal(again.depth, batched[name].depth) and torch.equal(again.confidence, batched[name].confidence)


def test_other_configurations_are_refused(golden, blob):
    from gtsfm_amd import native

    with pytest.raises(native.NativeError):
        _run(golden["a"], blob, config=native.PatchmatchNetConfig(iterations=(1, 2, 3)))
    _run(golden["a"], blob, config=native.PatchmatchNetConfig())
