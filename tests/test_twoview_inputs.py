"""CPU companion of tests/test_twoview_inputs_gpu.py and of the F-path edge tests: oracle only.

The GPU tests compare the two-view kernels with the oracle on a packed batch (tests/twoview_batch.py) under the
reference's conventions: side k normalised with image k's K, threshold thr_px / max(f1, f2)
(opencv_verifier_base.py:86), E = K2^T F K1 (utils/verification.py:110), column k of the match indices indexing image
k. That comparison can only catch a kernel that uses another convention if the other convention changes the answer on
these inputs. Here each wrong convention is fed to the oracle and must come out visibly different -- another inlier
mask, or a rotation more than 1 degree away -- on every pair it applies to, and the right one must recover the ground
truth. The oracle-side facts the F-path edge tests lean on (degenerate inputs give no model; the noisy LMedS pairs have a
positive median, and at M = 14 a threshold above the 0.001 floor) are pinned here too.
"""
import ctypes

import numpy as np
import pytest

from tests import scenes, twoview_batch as tb

F_MAX_ITERS = tb.F_MAX_ITERS


@pytest.fixture(scope="module")
def std():
    return tb.standard_batch("wide")


def _e_path(oracle, b, p, conv="correct"):
    """oracle.ransac_E on pair p under a convention: (mask, R) or None."""
    K1, K2, x1, x2 = b.K1[p], b.K2[p], b.x1[p], b.x2[p]
    div = {"thr_min": min(K1[0], K2[0]), "thr_f1": K1[0], "thr_f2": K2[0]}.get(conv, max(K1[0], K2[0]))
    if conv == "swapped_intrinsics":
        K1, K2 = K2, K1
    if conv == "swapped_columns":
        x1, x2 = _gather_swapped(b, p)
    r = oracle.ransac_E(tb.normalise(x1, K1), tb.normalise(x2, K2), tb.THR_PX / div, pair_id=tb.PAIR_IDS[p])
    return None if r is None else (r[1], r[2])


def _f_path(oracle, b, p, conv="correct"):
    """oracle.ransac_F + E + recover_pose on pair p under a convention: (mask, R) or None."""
    K1, K2, x1, x2 = b.K1[p], b.K2[p], b.x1[p], b.x2[p]
    if conv == "swapped_intrinsics":
        K1, K2 = K2, K1
    if conv == "swapped_columns":
        x1, x2 = _gather_swapped(b, p)
    r = oracle.ransac_F(x1, x2, tb.THR_PX, max_iters=F_MAX_ITERS, pair_id=tb.PAIR_IDS[p])
    if r is None:
        return None
    F, mask = r[0], r[1]
    M1, M2 = tb.k_matrix(K1), tb.k_matrix(K2)
    E = M1.T @ F @ M2 if conv == "k1t_f_k2" else M2.T @ F @ M1
    sel = mask.astype(bool)
    R, _, _ = oracle.recover_pose(E, tb.normalise(x1, K1)[sel], tb.normalise(x2, K2)[sel])
    return mask, R


def _gather_swapped(b, p):
    """What a kernel reads if it indexes image 1 with column 1 and image 2 with column 0."""
    i1, i2 = b.pairs[p]
    mi = b.match_idx[p, : b.match_count[p]]
    return b.kp[i1][mi[:, 1]], b.kp[i2][mi[:, 0]]


def _differs(wrong, right) -> bool:
    if wrong is None:
        return True
    return (not np.array_equal(wrong[0], right[0])) or scenes.rotation_angle_deg(wrong[1], right[1]) > 1.0


def test_packed_batch_layout():
    """The properties of the packed batch that make its indices non-trivial, for both layouts."""
    wide, tall = tb.standard_batch("wide")[0], tb.standard_batch("tall")[0]
    assert wide.kmax > wide.mcap and tall.kmax < tall.mcap
    for b in (wide, tall):
        P, n_img = len(b.pairs), len(b.intr)
        assert n_img == 5 and P >= 7
        first, second = set(b.pairs[:, 0].tolist()), set(b.pairs[:, 1].tolist())
        assert all(np.count_nonzero(b.pairs == i) > 1 for i in range(n_img))
        assert first & second
        assert np.count_nonzero(b.pairs[:, 0] > b.pairs[:, 1]) >= 2
        assert any(b.K1[p] == b.K2[p] for p in range(P)) and sum(b.K1[p] != b.K2[p] for p in range(P)) >= 6
        # threshold divisors: pairs with f1 < f2 and with f1 > f2 both occur
        assert sum(b.K1[p][0] < b.K2[p][0] for p in range(P)) >= 2
        assert sum(b.K1[p][0] > b.K2[p][0] for p in range(P)) >= 2
        assert np.isfinite(b.kp).all()
        assert b.match_idx.min() >= 0 and b.match_idx.max() < b.kmax
        for i in range(n_img):
            assert b.n_slots[i] < b.kmax and (b.kp[i, b.n_slots[i]:] == np.float32(tb.DECOY)).all()
            assert (np.abs(b.kp[i, : b.n_slots[i]]) < 1e5).all()
        for p in range(P):
            (i1, i2), M = b.pairs[p], b.match_count[p]
            live, pad = b.match_idx[p, :M], b.match_idx[p, M:]
            assert len(pad) > 0 and (pad[:, 0] >= b.n_slots[i1]).all() and (pad[:, 1] >= b.n_slots[i2]).all()
            for col in (0, 1):  # a permutation of a block, not the identity, and not the other column's order
                c = np.sort(live[:, col])
                assert np.array_equal(c, np.arange(c[0], c[0] + M)) and not np.array_equal(live[:, col], c)
            assert not np.array_equal(live[:, 0] - live[:, 0].min(), live[:, 1] - live[:, 1].min())
            # the expected inputs are the packed ones (checked here once; the tests never gather again)
            assert np.array_equal(b.kp[i1][live[:, 0]], b.x1[p]) and np.array_equal(b.kp[i2][live[:, 1]], b.x2[p])
    # the same pixels in both layouts, packed differently
    for p in range(len(wide.pairs)):
        assert np.array_equal(np.sort(wide.x1[p], axis=0), np.sort(tall.x1[p], axis=0))
    assert not np.array_equal(wide.match_idx[:, :40], tall.match_idx[:, :40])


def test_correct_convention_recovers_ground_truth(oracle_mod, std):
    b, gt = std
    n_e = n_f = 0
    for p in range(len(b.pairs)):
        mask, R = _e_path(oracle_mod, b, p)
        if mask.sum() >= 50:
            n_e += 1
            assert scenes.rotation_angle_deg(R, gt[p][0]) < 2.0, p
        mask, R = _f_path(oracle_mod, b, p)
        if mask.sum() >= 50:
            n_f += 1
            assert scenes.rotation_angle_deg(R, gt[p][0]) < 3.0, p
    assert n_e >= 6 and n_f >= 6  # the bars above are not vacuous


def _applies(conv, K1, K2) -> bool:
    """A wrong convention can only show where it differs from the right one: any of them needs K1 != K2, and a single
    focal length as the divisor is the right one, max(f1, f2), on the pairs where it is the larger."""
    if K1 == K2:
        return False
    if conv == "thr_min":
        return K1[0] != K2[0]
    if conv == "thr_f1":
        return K1[0] < K2[0]
    if conv == "thr_f2":
        return K2[0] < K1[0]
    return True


@pytest.mark.parametrize("conv", ["swapped_intrinsics", "thr_min", "thr_f1", "thr_f2", "swapped_columns"])
def test_wrong_convention_is_visible_on_E_path(oracle_mod, std, conv):
    b, _ = std
    pairs = [p for p in range(len(b.pairs)) if _applies(conv, b.K1[p], b.K2[p])]
    assert len(pairs) >= 2
    for p in pairs:
        assert _differs(_e_path(oracle_mod, b, p, conv), _e_path(oracle_mod, b, p)), (conv, p)


@pytest.mark.parametrize("conv", ["swapped_intrinsics", "k1t_f_k2", "swapped_columns"])
def test_wrong_convention_is_visible_on_F_path(oracle_mod, std, conv):
    b, _ = std
    pairs = [p for p in range(len(b.pairs)) if _applies(conv, b.K1[p], b.K2[p])]
    assert len(pairs) >= 6
    for p in pairs:
        assert _differs(_f_path(oracle_mod, b, p, conv), _f_path(oracle_mod, b, p)), (conv, p)


def test_swapped_columns_visible_with_equal_intrinsics(oracle_mod, std):
    """The column mix-up does not need K1 != K2: the control pair shows it too."""
    b, _ = std
    for p in range(len(b.pairs)):
        if b.K1[p] == b.K2[p]:
            assert _differs(_e_path(oracle_mod, b, p, "swapped_columns"), _e_path(oracle_mod, b, p))
            assert _differs(_f_path(oracle_mod, b, p, "swapped_columns"), _f_path(oracle_mod, b, p))


def test_degenerate_F_inputs_give_no_model(oracle_mod):
    """ransac_F returns None on them and does not expose its hypothesis count then, so the GPU test asserts none."""
    for a, b in tb.f_degenerate_pairs():
        assert len(a) == 30
        assert oracle_mod.ransac_F(a, b, 4.0, max_iters=F_MAX_ITERS, pair_id=0) is None
    a, b = tb.f_edge_pairs()[0]
    assert len(a) == 7 and oracle_mod.ransac_F(a, b, 4.0, max_iters=F_MAX_ITERS, pair_id=0) is None


def test_noisy_lmeds_pairs_have_positive_median(oracle_mod):
    """The least median over every candidate of every hypothesis LMedS can draw (a superset: 1024 >= the 960 it
    draws at the default confidence) is positive on both noisy LMedS pairs. At M = 14 the median is the 8th smallest
    error, one beyond the seven points the model interpolates, and the threshold derived from it is above the 0.001
    floor. At M = 8 (any M < 14) the median is the error of one of the seven sample points: rounding-level whatever
    the noise, so that pair's threshold is the floor by construction of the algorithm, and only M = 14 covers the
    branch above it."""
    L = oracle_mod.lib()
    # keyed like the GPU test's launch: pair id = position among the edge pairs
    pairs = [(pid, a, b) for pid, (a, b) in enumerate(tb.f_edge_pairs()) if 8 <= len(a) < 15]
    assert [len(a) for _, a, _ in pairs] == [8, 14]
    for pid, a, b in pairs:
        M = len(a)
        pts = np.ascontiguousarray(np.hstack([a, b]), np.float32)
        idx = np.zeros(7, np.int32)
        min_median, n_models = np.inf, 0
        for h in range(1024):
            if not L.oracle_sample7(ctypes.c_uint64(oracle_mod.RANSAC_SEED), pid, h, M, pts.ravel(), idx):
                continue
            for F in oracle_mod.seven_point(a[idx], b[idx]):
                n_models += 1
                min_median = min(min_median, float(np.sort(oracle_mod.f_errors(F, a, b))[M // 2]))
        assert n_models > 0 and min_median > 0.0
        thr = 2.5 * 1.4826 * (1.0 + 5.0 / (M - 7)) * np.sqrt(min_median)
        assert (thr > 0.001) if M // 2 >= 7 else (thr < 0.001), (M, min_median, thr)
