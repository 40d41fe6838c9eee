"""GPU fundamental-matrix verifier (gtsfm_ransac_F_batched, Ransac(use_intrinsics_in_verification=False)).

Known answer: the reference's TestRansacForFundamentalMatrix two-plane scene (tests/frontend/verifier/test_ransac.py
:22-30 over test_verifier_base.py:81-100): all 8 putatives verified, R and t within 2 deg.
Oracle parity (oracle/fundamental.c): both compute the same double operations in the same order without FMA
contraction, so F, the inlier mask, the inlier count and the hypothesis count are bit-identical; R/t come from the
recoverPose shared with the E path (twoview.hpp recover_pose, also compiled without contraction) and are checked
within 1e-9 per entry.
"""
import numpy as np
import pytest
import torch

from tests import scenes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from gtsfm_amd import native

    native.require_gpu()
    native.lib()
    return torch.device("cuda")


def _kp(xy):
    from gtsfm_amd.common.keypoints import Keypoints

    return Keypoints(coordinates=np.asarray(xy, dtype=np.float64))


def test_two_plane_scene_F_path(dev):
    from gtsfm_amd.common import geometry
    from gtsfm_amd.frontend.verifier.ransac import Ransac

    uv1, uv2, R, t = scenes.two_planes_scene(4, 4)
    match = np.vstack((np.arange(8), np.arange(8))).T
    v = Ransac(use_intrinsics_in_verification=False, estimation_threshold_px=0.5)
    Rc, Uc, idx, ratio = v.verify(_kp(uv1), _kp(uv2), match, geometry.Cal3Bundler(), geometry.Cal3Bundler())
    np.testing.assert_array_equal(idx, match)
    assert ratio == 1.0
    assert scenes.rotation_angle_deg(R, geometry.rotation_matrix(Rc)) < 2
    assert scenes.direction_angle_deg(t, geometry.unit_vector(Uc)) < 2


def test_F_too_few_matches(dev):
    from gtsfm_amd.common import geometry
    from gtsfm_amd.frontend.verifier.ransac import Ransac

    rng = np.random.default_rng(0)
    kp1, kp2, K, R, t, _ = scenes.random_two_view(rng, 7, 0)
    v = Ransac(use_intrinsics_in_verification=False, estimation_threshold_px=4)
    cal = geometry.Cal3Bundler(K[0, 0], 0, 0, K[0, 2], K[1, 2])
    out = v.verify(_kp(kp1), _kp(kp2), np.vstack([np.arange(7)] * 2).T, cal, cal)
    assert out[0] is None and out[1] is None and out[2].dtype == np.uint64 and out[3] == 0.0


def test_F_batched_bit_exact_vs_oracle(dev, oracle_mod):
    from gtsfm_amd import device, native

    rng = np.random.default_rng(21)
    n_pairs = 24
    kps, Ks, Ms, gts = [], [], [], []
    for p in range(n_pairs):
        if p % 6 == 0:  # LMedS branch (8 <= M < 15), noise-free
            kp1, kp2, K, R, t, inl = scenes.random_two_view(rng, int(rng.integers(8, 15)), 0, noise_px=0.0)
        else:
            n_in = int(rng.integers(20, 500))
            kp1, kp2, K, R, t, inl = scenes.random_two_view(rng, n_in, int(n_in * rng.uniform(0.2, 1.2)))
        kps.append((kp1.astype(np.float32), kp2.astype(np.float32)))
        Ks.append(K)
        Ms.append(len(kp1))
        gts.append((R, t))
    kmax = max(Ms)
    kp = np.zeros((2 * n_pairs, kmax, 2), np.float32)
    intr = np.zeros((2 * n_pairs, 3))
    pairs = np.zeros((n_pairs, 2), np.int32)
    mi = np.zeros((n_pairs, kmax, 2), np.int32)
    for p, ((a, b), K) in enumerate(zip(kps, Ks)):
        kp[2 * p, : len(a)], kp[2 * p + 1, : len(b)] = a, b
        intr[2 * p] = intr[2 * p + 1] = (K[0, 0], K[0, 2], K[1, 2])
        pairs[p] = (2 * p, 2 * p + 1)
        mi[p, : Ms[p]] = np.arange(Ms[p])[:, None]
    res = device.ransac_fundamental(torch.from_numpy(kp).to(dev), torch.from_numpy(intr).to(dev),
                                    torch.from_numpy(pairs).to(dev), torch.from_numpy(mi).to(dev),
                                    torch.tensor(Ms, dtype=torch.int32, device=dev), 4.0, max_iters=200000)
    st, n_inl, n_hyp = res.status.cpu().numpy(), res.n_inliers.cpu().numpy(), res.n_hyp.cpu().numpy()
    F, E, R, t, mask = (res.F.cpu().numpy(), res.E.cpu().numpy(), res.R.cpu().numpy(), res.t.cpu().numpy(),
                        res.mask.cpu().numpy())
    for p in range(n_pairs):
        a, b = kps[p]
        K = Ks[p]
        ref = oracle_mod.ransac_F(a, b, 4.0, max_iters=200000, pair_id=p)
        assert ref is not None and st[p] == native.RANSAC_STATUS_OK, p
        rF, rmask, rn, rnh = ref
        assert np.array_equal(F[p], rF), (p, F[p], rF)
        assert np.array_equal(mask[p, : Ms[p]], rmask), p
        assert n_inl[p] == rn and n_hyp[p] == rnh, p
        np.testing.assert_allclose(E[p], K.T @ rF @ K, rtol=1e-12, atol=1e-12 * np.abs(E[p]).max())
        sel = rmask.astype(bool)
        rR, rt, _ = oracle_mod.recover_pose(K.T @ rF @ K, (a[sel].astype(np.float64) - K[:2, 2]) / K[0, 0],
                                            (b[sel].astype(np.float64) - K[:2, 2]) / K[0, 0])
        np.testing.assert_allclose(R[p], rR, atol=1e-9)
        np.testing.assert_allclose(t[p], rt, atol=1e-9)
        if rn >= 50:
            assert scenes.rotation_angle_deg(R[p], gts[p][0]) < 3.0, p


def test_F_batch_equals_single_pair_calls(dev):
    from gtsfm_amd.common import geometry
    from gtsfm_amd.frontend.verifier.ransac import Ransac

    rng = np.random.default_rng(4)
    v = Ransac(use_intrinsics_in_verification=False, estimation_threshold_px=4)
    kps, corr, cals = [], {}, []
    for p in range(4):
        kp1, kp2, K, R, t, _ = scenes.random_two_view(rng, 150, 100)
        kps += [_kp(kp1), _kp(kp2)]
        cal = geometry.Cal3Bundler(K[0, 0], 0, 0, K[0, 2], K[1, 2])
        cals += [cal, cal]
        corr[(2 * p, 2 * p + 1)] = np.vstack([np.arange(len(kp1))] * 2).T.astype(np.uint32)
    batch = v.verify_batch(kps, corr, cals)
    for (i1, i2), m in corr.items():
        single = v.verify(kps[i1], kps[i2], m, cals[i1], cals[i2])
        assert np.array_equal(batch[(i1, i2)][2], single[2])
        assert np.array_equal(geometry.rotation_matrix(batch[(i1, i2)][0]), geometry.rotation_matrix(single[0]))


# ---- edges: putative counts on the LMedS / wave boundaries, max_iters off the batch size, degenerate pairs ----------
# Inputs from tests/twoview_batch.py (tests/test_twoview_inputs.py pins what the oracle does on them). Columns of the
# mask at or past match_count[p] are not compared: the header does not define them.

def _run_F(dev, pairs_xy, **kw):
    from gtsfm_amd import device
    from tests import twoview_batch as tb

    kp, intr, pairs, mi, cnt = tb.pack_private(pairs_xy)
    res = device.ransac_fundamental(torch.from_numpy(kp).to(dev), torch.from_numpy(intr).to(dev),
                                    torch.from_numpy(pairs).to(dev), torch.from_numpy(mi).to(dev),
                                    torch.from_numpy(cnt).to(dev), 4.0, **kw)
    return {k: getattr(res, k).cpu().numpy() for k in ("status", "n_inliers", "n_hyp", "F", "mask")}


def _assert_F_pair_equals_oracle(g, p, ref, M):
    """Pair p of a launch against oracle.ransac_F's result for it (None = no model)."""
    from gtsfm_amd import native

    if ref is None:
        assert g["status"][p] == native.RANSAC_STATUS_NO_MODEL, (p, g["status"][p])
        assert g["n_inliers"][p] == 0 and not g["mask"][p, :M].any(), p
        return
    rF, rmask, rn, rnh = ref
    assert g["status"][p] == native.RANSAC_STATUS_OK, (p, g["status"][p])
    assert np.array_equal(g["F"][p], rF), (p, g["F"][p], rF)
    assert np.array_equal(g["mask"][p, :M], rmask), p
    assert g["n_inliers"][p] == rn and g["n_hyp"][p] == rnh, (p, g["n_inliers"][p], rn, g["n_hyp"][p], rnh)


def test_F_putative_counts_on_the_boundaries(dev, oracle_mod):
    """M = 7, 8, 14 (LMedS, noisy, two gross outliers), 15, 16 (first RANSAC sizes), 63, 64, 65, 128, 129 (wave
    boundaries), one launch."""
    from gtsfm_amd import native
    from tests import twoview_batch as tb

    pairs_xy = tb.f_edge_pairs()
    assert tuple(len(a) for a, _ in pairs_xy) == tb.F_EDGE_COUNTS
    g = _run_F(dev, pairs_xy, max_iters=200000)
    n_ok = 0
    for p, (a, b) in enumerate(pairs_xy):
        M = len(a)
        if M == 7:
            assert g["status"][p] == native.RANSAC_STATUS_TOO_FEW
            assert g["n_inliers"][p] == 0 and g["n_hyp"][p] == 0 and not g["mask"][p, :M].any()
            continue
        ref = oracle_mod.ransac_F(a, b, 4.0, max_iters=200000, pair_id=p)
        _assert_F_pair_equals_oracle(g, p, ref, M)
        n_ok += ref is not None
        if M >= 15:
            assert ref is not None, M
    assert n_ok >= 8


@pytest.mark.parametrize("max_iters", [1, 64, 65, 100])
def test_F_max_iters_off_the_batch_size(dev, oracle_mod, max_iters):
    from tests import twoview_batch as tb

    a, b = tb.f_max_iters_pair()
    g = _run_F(dev, [(a, b)], max_iters=max_iters)
    ref = oracle_mod.ransac_F(a, b, 4.0, max_iters=max_iters, pair_id=0)
    assert ref is not None
    _assert_F_pair_equals_oracle(g, 0, ref, len(a))
    assert g["n_hyp"][0] == ref[3] and g["n_hyp"][0] % 64 == 0 and g["n_hyp"][0] >= max_iters


def test_F_degenerate_pairs_give_no_model(dev, oracle_mod):
    """All putatives on a line in image 1, and all at one point in both images: status NO_MODEL, no inliers, an
    all-zero mask (the oracle does not report its hypothesis count without a model, so none is compared); the ordinary
    pairs before, between and after them in the launch still equal the oracle."""
    from tests import twoview_batch as tb

    line, point = tb.f_degenerate_pairs()
    pairs_xy = [tb.f_ordinary_pair(1), line, tb.f_ordinary_pair(2), point, tb.f_ordinary_pair(3)]
    g = _run_F(dev, pairs_xy, max_iters=200000)
    for p, (a, b) in enumerate(pairs_xy):
        ref = oracle_mod.ransac_F(a, b, 4.0, max_iters=200000, pair_id=p)
        assert (ref is None) == (p in (1, 3)), p
        _assert_F_pair_equals_oracle(g, p, ref, len(a))
