"""LightGlue on the GPU (gtsfm_lightglue_batched through the C ABI) against the float64 restatement
(tests/lightglue_ref.py) on the cases of tests/lightglue_cases.py.

Bars (lightglue_cases.bars()): |dZ| on live entries (Z_ref > -20) and |dscore| at most 4 x the float32
restatement's own maxima over the same cases (MEASURED); dead entries below -15; matches identical except at near-ties
(row, column or threshold margin below 2 x the Z bar on the GPU's own Z), at most max(2, 2 %) of the reference's
matches; exit layers exactly the reference's (tests/test_lightglue_ref.py shows every stop decision to be robust).
"""
import numpy as np
import pytest
import torch

import lightglue_cases as lc
from superglue_cases import kmax_of, near_tie_margins

pytestmark = pytest.mark.gpu

Z_BAR, SCORE_BAR = lc.bars()


@pytest.fixture(scope="module")
def weights():
    from gtsfm_amd.frontend.matcher.lightglue_matcher import pack_lightglue_weights

    return torch.from_numpy(pack_lightglue_weights(lc.state_dict())).cuda()


def _compare(name, ref, Z, matches0, mscores0, rows=None):
    """One pair of a GPU run against its float64 reference (rows: the subset of Z's rows to compare)."""
    rows = np.arange(ref.Z.shape[0]) if rows is None else rows
    Zr, Zg = ref.Z[rows], Z[rows].astype(np.float64)
    assert np.isfinite(Zg).all()
    live = Zr > -20
    dz = float(np.abs(Zg - Zr)[live].max())
    ds = float(np.abs(mscores0 - ref.mscores0).max())
    print(f"{name}: |dZ| {dz:.2e} (bar {Z_BAR:.2e})  |dscore| {ds:.2e} (bar {SCORE_BAR:.2e})")
    assert dz <= Z_BAR, (name, dz, Z_BAR)
    assert (Zg[~live] < -15).all()
    assert ds <= SCORE_BAR, (name, ds, SCORE_BAR)
    margins = near_tie_margins(Z[:-1, :-1], matches0, ref.matches0, 0.1)
    assert len(margins) <= max(2, 0.02 * len(ref.matches)), (name, margins)
    assert all(m < 2 * Z_BAR for m in margins.values()), (name, margins)


@pytest.mark.parametrize("depth_confidence", [0.95, -1.0])
@pytest.mark.parametrize("shape", lc.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_single_pair(weights, shape, depth_confidence):
    name = f"{shape[0]}x{shape[1]}"
    a, b = lc.cases()[name]
    assert a.hw != b.hw
    ref = lc.reference_of(name, depth_confidence)
    run = lc.run_gpu([a, b], [(0, 1)], weights, depth_confidence=depth_confidence)
    assert int(run.exit_layer[0]) == ref.exit_layer
    if depth_confidence < 0:
        assert int(run.exit_layer[0]) == 8
    _compare(name, ref, run.Z[0], run.matches0[0], run.mscores0[0])
    # emitted in ascending first index
    assert (np.diff(run.pairs_out[0][:, 0].astype(np.int64)) > 0).all()


def test_each_side_is_normalised_by_its_own_image_size(weights):
    a, b = lc.cases()["128x129"]
    sa, sb = lc.cases()["128x129_hw_swapped"]
    np.testing.assert_array_equal(a.desc, sa.desc)
    assert (sa.hw, sb.hw) == (b.hw, a.hw)
    ref, ref_sw = lc.reference_of("128x129"), lc.reference_of("128x129_hw_swapped")
    # not vacuous: the same keypoints under the other image sizes give another answer
    moved = lc.reference(a._replace(hw=b.hw), b._replace(hw=a.hw))
    assert np.abs(moved.Z - ref.Z)[ref.Z > -20].max() > 100 * Z_BAR
    run = lc.run_gpu([sa, sb], [(0, 1)], weights)
    assert int(run.exit_layer[0]) == ref_sw.exit_layer
    _compare("128x129_hw_swapped", ref_sw, run.Z[0], run.matches0[0], run.mscores0[0])


@pytest.fixture(scope="module")
def depth_run(weights):
    return lc.run_gpu(lc.make_depth_images(), lc.DEPTH_PAIRS, weights, kmax=lc.DEPTH_KMAX)


def test_batched_adaptive_depth_against_reference(depth_run):
    refs = [lc.reference_of(f"depth_{i}_{j}") for i, j in lc.DEPTH_PAIRS]
    assert depth_run.exit_layer.tolist() == [r.exit_layer for r in refs]
    assert len(set(depth_run.exit_layer.tolist())) >= 3
    for q, (i, j) in enumerate(lc.DEPTH_PAIRS):
        _compare(f"depth_{i}_{j}", refs[q], depth_run.Z[q], depth_run.matches0[q], depth_run.mscores0[q])


def test_batched_pairs_use_their_own_layers_assignment_weights(depth_run):
    """A pair that stops at layer 0 beside pairs that stop later: under another layer's final_proj / matchability the
    reference moves by far more than the bar, and the GPU stays with the right one."""
    q = lc.DEPTH_PAIRS.index((0, 1))
    ref = lc.reference_of("depth_0_1")
    assert ref.exit_layer == 0
    im = lc.make_depth_images()
    live = ref.Z > -20
    for other in sorted(set(depth_run.exit_layer.tolist()) - {0}):
        wrong = lc.reference(im[0], im[1], assign_layer=int(other))
        assert np.abs(wrong.Z - ref.Z)[live].max() > 100 * Z_BAR
    assert np.abs(depth_run.Z[q] - ref.Z)[live].max() <= Z_BAR


def test_batched_pairs_are_bitwise_what_they_give_alone(weights, depth_run):
    im = lc.make_depth_images()
    for q, (i, j) in enumerate(lc.DEPTH_PAIRS):
        alone = lc.run_gpu([im[i], im[j]], [(0, 1)], weights, kmax=lc.DEPTH_KMAX)
        assert int(alone.exit_layer[0]) == int(depth_run.exit_layer[q])
        np.testing.assert_array_equal(alone.Z[0], depth_run.Z[q])
        np.testing.assert_array_equal(alone.pairs_out[0], depth_run.pairs_out[q])
        np.testing.assert_array_equal(alone.mscores0[0], depth_run.mscores0[q])


def test_reduction_kernels_loop_more_than_once(weights):
    """kmax 576, both counts above 512: the row log-sum-exp pass takes 256 columns per step and the column pass 16
    rows, so both loop at least three times (and the LayerNorm row kernel runs over 2 x 1090 rows)."""
    a, b = lc.cases()["loop_560x530"]
    assert lc.LOOP_KMAX == kmax_of(len(a.kp), len(b.kp)) and min(len(a.kp), len(b.kp)) > 2 * 256
    ref = lc.reference_of("loop_560x530")
    run = lc.run_gpu([a, b], [(0, 1)], weights, kmax=lc.LOOP_KMAX)
    assert int(run.exit_layer[0]) == ref.exit_layer
    rows = np.unique(np.concatenate([np.arange(0, len(a.kp), 16), [len(a.kp)]]))
    _compare("loop_560x530", ref, run.Z[0], run.matches0[0], run.mscores0[0], rows=rows)


def test_identical_columns_match_the_lower_index(weights):
    a, b, lo, hi = lc.make_tie_pair()
    ref = lc.reference(a, b)
    run = lc.run_gpu([a, b], [(0, 1)], weights)
    np.testing.assert_array_equal(run.Z[0][:, lo], run.Z[0][:, hi])
    got = run.pairs_out[0]
    assert lo in got[:, 1] and hi not in got[:, 1]
    i = int(ref.matches[ref.matches[:, 1] == lo][0, 0])
    assert run.matches0[0][i] == lo


def test_empty_sides_and_no_pairs(weights):
    from superglue_cases import make_side

    a, b = lc.cases()["15x17"]
    empty = make_side(np.random.default_rng(0), 0, (480, 640))
    run = lc.run_gpu([a, empty, b], [(0, 1), (0, 2), (1, 2), (1, 1)], weights, kmax=64)
    assert [len(p) for p in run.pairs_out] == [0, len(lc.reference_of("15x17").matches), 0, 0]
    alone = lc.run_gpu([a, b], [(0, 1)], weights, kmax=64)
    np.testing.assert_array_equal(run.pairs_out[1], alone.pairs_out[0])
    none = lc.run_gpu([a, b], [], weights, kmax=64)
    assert none.pairs_out == [] and len(none.exit_layer) == 0


def test_entry_point_argument_checks(weights):
    from gtsfm_amd import native

    L = native.lib()
    assert L.gtsfm_lightglue_weights_floats(0) == 0 and L.gtsfm_lightglue_workspace_bytes(0, 64) == 0
    assert L.gtsfm_lightglue_workspace_bytes(3, 0) == 0
    kmax = 64
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device="cuda")  # noqa: E731
    kp, de, cnt, hw = z(2, kmax, 2), z(2, kmax, 256), z(2, dt=torch.int32), z(2, 2, dt=torch.int32)
    pairs, idx, oc = z(1, 2, dt=torch.int32), z(1, kmax, 2, dt=torch.int32), z(1, dt=torch.int32)
    ws = torch.empty(L.gtsfm_lightglue_workspace_bytes(1, kmax), dtype=torch.uint8, device="cuda")
    p = lambda t: t.data_ptr()  # noqa: E731

    def call(kp_=None, kmax_=kmax, n_pairs=1, n_layers=9, ws_bytes=None, idx_=None):
        return L.gtsfm_lightglue_batched(p(kp) if kp_ is None else kp_, p(de), p(cnt), p(hw), 2, kmax_, p(pairs),
                                         n_pairs, p(weights), n_layers, 0.95, 0.1, p(ws),
                                         ws.numel() if ws_bytes is None else ws_bytes, p(idx) if idx_ is None else idx_,
                                         p(oc), None, None, native.stream_handle())

    assert call(n_pairs=0) == native.GTSFM_OK
    assert call() == native.GTSFM_OK  # both sides empty: nothing runs, no matches
    torch.cuda.synchronize()
    assert int(oc[0]) == 0
    assert call(kp_=0) == native.GTSFM_ERR_ARG
    assert call(idx_=0) == native.GTSFM_ERR_ARG
    assert call(kmax_=65) == native.GTSFM_ERR_ARG
    assert call(n_pairs=-1) == native.GTSFM_ERR_ARG
    assert call(n_layers=0) == native.GTSFM_ERR_ARG
    assert call(ws_bytes=ws.numel() - 1) == native.GTSFM_ERR_CAPACITY
    out = z(kmax + 1, kmax + 1)
    assert L.gtsfm_lightglue_log_assignment(p(ws), ws.numel(), 1, kmax, 1, p(out), native.stream_handle()) == native.GTSFM_ERR_ARG
    assert L.gtsfm_lightglue_log_assignment(p(ws), ws.numel(), 1, kmax, 0, 0, native.stream_handle()) == native.GTSFM_ERR_ARG


def test_generator_batches_superpoint_and_lightglue_like_per_call_match():
    from gtsfm_amd import synthetic
    from gtsfm_amd.common.image import Image
    from gtsfm_amd.frontend.correspondence_generator.det_desc_correspondence_generator import \
        DetDescCorrespondenceGenerator
    from gtsfm_amd.frontend.detector_descriptor.superpoint import SuperPointDetectorDescriptor
    from gtsfm_amd.frontend.matcher.lightglue_matcher import LightGlueMatcher
    from superpoint_weights import superpoint_state_dict

    arr = synthetic.render_scene(32, 240, 320, device="cuda", indices=[0, 1, 2]).images.cpu().numpy()
    sp = SuperPointDetectorDescriptor(max_keypoints=192, state_dict=superpoint_state_dict(0, whitened=True))
    lg = LightGlueMatcher("superpoint", state_dict=lc.state_dict())
    imgs = [Image(a) for a in arr]
    pairs = [(0, 1), (0, 2), (1, 2)]
    gen = DetDescCorrespondenceGenerator(lg, sp)
    assert gen._batched() == "superpoint_lightglue"
    kps, corr = gen.generate_correspondences(None, imgs, pairs)
    per = [sp.detect_and_describe(im) for im in imgs]
    total = 0
    for i1, i2 in pairs:
        ref = lg.match(per[i1][0], per[i2][0], per[i1][1], per[i2][1], arr[i1].shape, arr[i2].shape)
        got = np.asarray(corr[(i1, i2)]).reshape(-1, 2)
        np.testing.assert_array_equal(got, np.asarray(ref).reshape(-1, 2))
        total += len(got)
    assert min(len(k) for k in kps) > 0 and total > 0
