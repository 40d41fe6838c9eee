"""The two-view entry points on a packed batch with per-image intrinsics (tests/twoview_batch.py) against the oracle.

gtsfm_ransac_E_batched, gtsfm_ransac_F_batched and gtsfm_ba2_batched each take one batched call over eight pairs that
share five images with four different calibrations, keypoint slots and putative rows permuted independently,
kmax != mcap (both ways round) and decoys wherever a correct kernel does not read. The oracle gets each pair's pixels
in putative order, each side normalised with its own K, the threshold thr_px / max(f1, f2), E = K2^T F K1 and explicit
non-sequential sampler keys; the bars are the ones of test_verifier_gpu.py, test_fundamental_gpu.py and
test_ba2_gpu.py. tests/test_twoview_inputs.py shows that every other convention changes the oracle's answer on these
inputs, so a kernel using one fails here. The Ransac plugin is checked against the device level on the same pairs.
"""
import numpy as np
import pytest
import torch

from tests import ba2_scenes, scenes, twoview_batch as tb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from gtsfm_amd import native

    native.require_gpu()
    native.lib()
    return torch.device("cuda")


@pytest.fixture(scope="module")
def batches():
    return {layout: tb.standard_batch(layout) for layout in tb.LAYOUTS}


@pytest.fixture(scope="module")
def e_refs(oracle_mod, batches):
    """oracle.ransac_E per layout and pair, computed once: (E, mask, R, t, n, n_hyp)."""
    out = {}
    for layout, (b, _) in batches.items():
        out[layout] = [oracle_mod.ransac_E(tb.normalise(b.x1[p], b.K1[p]), tb.normalise(b.x2[p], b.K2[p]),
                                           tb.THR_PX / max(b.K1[p][0], b.K2[p][0]), pair_id=tb.PAIR_IDS[p])
                       for p in range(len(b.pairs))]
    return out


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _args(b, dev):
    return _t(b.kp, dev), _t(b.intr, dev), _t(b.pairs, dev), _t(b.match_idx, dev), _t(b.match_count, dev)


def _ids(ids, dev):
    return torch.tensor(list(ids), dtype=torch.int32, device=dev)


def _host(res, names):
    return {k: getattr(res, k).cpu().numpy() for k in names}


def _assert_same_per_pair(fwd, rev, counts):
    """Outputs of a launch over the reversed batch, pair for pair byte-identical to the forward launch."""
    P = len(counts)
    for p in range(P):
        q = P - 1 - p
        for k in fwd:
            a, r = fwd[k][p], rev[k][q]
            if k == "mask":
                a, r = a[: counts[p]], r[: counts[p]]
            assert a.tobytes() == r.tobytes(), (k, p)


@pytest.mark.parametrize("layout", tb.LAYOUTS)
def test_E_path_packed_vs_oracle(dev, batches, e_refs, layout):
    from gtsfm_amd import device, native

    b, gt = batches[layout]
    res = device.ransac_essential(*_args(b, dev), tb.THR_PX, pair_ids=_ids(tb.PAIR_IDS, dev))
    names = ("status", "n_hyp", "n_inliers", "mask", "E", "R", "t")
    g = _host(res, names)
    n_acc = 0
    for p in range(len(b.pairs)):
        M = b.match_count[p]
        _, rmask, rR, rt, rn, rh = e_refs[layout][p]
        assert g["status"][p] == native.RANSAC_STATUS_OK, p
        assert int(g["n_hyp"][p]) == rh, (p, g["n_hyp"][p], rh)
        assert int(g["n_inliers"][p]) == rn, (p, g["n_inliers"][p], rn)
        np.testing.assert_array_equal(g["mask"][p, :M], rmask.astype(np.uint8))
        np.testing.assert_array_equal(g["R"][p], rR)
        np.testing.assert_array_equal(g["t"][p], rt)
        if rn >= 50:
            n_acc += 1
            assert scenes.rotation_angle_deg(g["R"][p], gt[p][0]) < 2.0, p
    assert n_acc >= 6
    # the same pairs in reverse order under the same sampler keys: nothing depends on a pair's place in the batch
    rb = b.reversed()
    rev = _host(device.ransac_essential(*_args(rb, dev), tb.THR_PX, pair_ids=_ids(tb.PAIR_IDS[::-1], dev)), names)
    _assert_same_per_pair(g, rev, b.match_count)


@pytest.mark.parametrize("layout", tb.LAYOUTS)
def test_F_path_packed_vs_oracle(dev, oracle_mod, batches, layout):
    from gtsfm_amd import device, native

    b, gt = batches[layout]
    res = device.ransac_fundamental(*_args(b, dev), tb.THR_PX, max_iters=tb.F_MAX_ITERS,
                                    pair_ids=_ids(tb.PAIR_IDS, dev))
    names = ("status", "n_hyp", "n_inliers", "mask", "F", "E", "R", "t")
    g = _host(res, names)
    n_acc = 0
    for p in range(len(b.pairs)):
        M, x1, x2, K1, K2 = b.match_count[p], b.x1[p], b.x2[p], b.K1[p], b.K2[p]
        ref = oracle_mod.ransac_F(x1, x2, tb.THR_PX, max_iters=tb.F_MAX_ITERS, pair_id=tb.PAIR_IDS[p])
        assert ref is not None and g["status"][p] == native.RANSAC_STATUS_OK, p
        rF, rmask, rn, rnh = ref
        assert np.array_equal(g["F"][p], rF), (p, g["F"][p], rF)
        assert np.array_equal(g["mask"][p, :M], rmask), p
        assert g["n_inliers"][p] == rn and g["n_hyp"][p] == rnh, p
        E = tb.k_matrix(K2).T @ rF @ tb.k_matrix(K1)
        np.testing.assert_allclose(g["E"][p], E, rtol=1e-12, atol=1e-12 * np.abs(g["E"][p]).max())
        sel = rmask.astype(bool)
        rR, rt, _ = oracle_mod.recover_pose(E, tb.normalise(x1, K1)[sel], tb.normalise(x2, K2)[sel])
        np.testing.assert_allclose(g["R"][p], rR, atol=1e-9)
        np.testing.assert_allclose(g["t"][p], rt, atol=1e-9)
        if rn >= 50:
            n_acc += 1
            assert scenes.rotation_angle_deg(g["R"][p], gt[p][0]) < 3.0, p
    assert n_acc >= 6
    rb = b.reversed()
    rev = _host(device.ransac_fundamental(*_args(rb, dev), tb.THR_PX, max_iters=tb.F_MAX_ITERS,
                                          pair_ids=_ids(tb.PAIR_IDS[::-1], dev)), names)
    _assert_same_per_pair(g, rev, b.match_count)


@pytest.mark.parametrize("layout", tb.LAYOUTS)
def test_ba2_packed_vs_oracle(dev, oracle_mod, batches, e_refs, layout):
    """gtsfm_ba2_batched fed with the E-path result of the same batch, against oracle.ba2 with K1 and K2 apart."""
    from gtsfm_amd import device

    b, gt = batches[layout]
    args = _args(b, dev)
    res = device.ransac_essential(*args, tb.THR_PX, pair_ids=_ids(tb.PAIR_IDS, dev))
    ba = device.bundle_adjust_2view(*args, res)
    g = _host(ba, ("ba_status", "iters", "R", "t", "mask", "n_inliers"))
    for p in range(len(b.pairs)):
        M = b.match_count[p]
        _, rmask, rR, rt, rn, _ = e_refs[layout][p]  # == the device's E-path result (test_E_path_packed_vs_oracle)
        rows = np.flatnonzero(rmask)
        assert len(rows) >= 15  # BA runs
        o_st, o_R, o_t, o_valid, o_it, _ = oracle_mod.ba2(b.x1[p][rows].astype(np.float64),
                                                          b.x2[p][rows].astype(np.float64), b.K1[p], b.K2[p], rR, rt)
        assert o_st == 0 and g["ba_status"][p] == o_st, (p, g["ba_status"][p], o_st)
        assert g["iters"][p] == o_it, (p, g["iters"][p], o_it)
        assert ba2_scenes.angle_deg(g["R"][p], o_R) < 1e-4 and ba2_scenes.dir_deg(g["t"][p], o_t) < 1e-4, p
        o_mask = np.zeros(M, np.uint8)
        o_mask[rows[o_valid]] = 1
        assert np.count_nonzero(g["mask"][p, :M] != o_mask) <= 1, p
        assert g["n_inliers"][p] == g["mask"][p, :M].sum()


def _kp(xy):
    from gtsfm_amd.common.keypoints import Keypoints

    return Keypoints(coordinates=np.asarray(xy, dtype=np.float64))


def _plugin_inputs(b):
    """Per image: its keypoints (the used slots and one decoy, so the images differ in length) and its Cal3Bundler."""
    from gtsfm_amd.common import geometry

    kps = [_kp(b.kp[i, : b.n_slots[i] + 1]) for i in range(len(b.intr))]
    cals = [geometry.Cal3Bundler(f, 0, 0, u0, v0) for f, u0, v0 in b.intr]
    return kps, cals


@pytest.mark.parametrize("use_intrinsics", [True, False])
def test_plugin_verify_equals_device_level(dev, batches, use_intrinsics):
    """Ransac.verify with two different Cal3Bundlers, as given and mirrored (image 2 as the first view), against the
    batched device call on the same pairs under verify()'s sampler key 0; verify_batch equals the single calls."""
    from gtsfm_amd import device
    from gtsfm_amd.common import geometry
    from gtsfm_amd.frontend.verifier import ransac as plugin

    b, _ = batches["wide"]
    P = len(b.pairs)
    v = plugin.Ransac(use_intrinsics_in_verification=use_intrinsics, estimation_threshold_px=tb.THR_PX)
    kps, cals = _plugin_inputs(b)
    zeros = _ids([0] * P, dev)
    kp_d, intr_d, pairs_d, mi_d, cnt_d = _args(b, dev)
    mirrored = (kp_d, intr_d, _t(b.pairs[:, ::-1], dev), _t(b.match_idx[:, :, ::-1], dev), cnt_d)
    singles = {}
    for flip, args in ((False, (kp_d, intr_d, pairs_d, mi_d, cnt_d)), (True, mirrored)):
        if use_intrinsics:
            res = device.ransac_essential(*args, tb.THR_PX, plugin.RANSAC_SUCCESS_PROB, plugin.RANSAC_MAX_ITERS,
                                          pair_ids=zeros)
        else:
            res = device.ransac_fundamental(*args, tb.THR_PX, plugin.RANSAC_SUCCESS_PROB, plugin.RANSAC_MAX_ITERS_F,
                                            pair_ids=zeros)
        g = _host(res, ("status", "mask", "R", "t"))
        for p in range(P):
            (i1, i2), M = (int(i) for i in b.pairs[p]), b.match_count[p]
            match = b.match_idx[p, :M].astype(np.uint32)
            if flip:
                i1, i2, match = i2, i1, np.ascontiguousarray(match[:, ::-1])
            R, U, idx, ratio = v.verify(kps[i1], kps[i2], match, cals[i1], cals[i2])
            assert g["status"][p] == 0 and R is not None, (flip, p)
            keep = g["mask"][p, :M].astype(bool)
            np.testing.assert_array_equal(idx, match[keep])
            np.testing.assert_array_equal(geometry.rotation_matrix(R), g["R"][p])
            assert ratio == float(np.mean(keep))
            if not flip:
                singles[(i1, i2)] = (R, U, idx, ratio)
    corr = {(int(b.pairs[p, 0]), int(b.pairs[p, 1])): b.match_idx[p, : b.match_count[p]].astype(np.uint32)
            for p in range(P)}
    batch = v.verify_batch(kps, corr, cals)
    assert set(batch) == set(singles)
    for key, (R, U, idx, ratio) in singles.items():
        assert np.array_equal(batch[key][2], idx) and batch[key][3] == ratio
        assert np.array_equal(geometry.rotation_matrix(batch[key][0]), geometry.rotation_matrix(R))
        assert np.array_equal(geometry.unit_vector(batch[key][1]), geometry.unit_vector(U))
