"""GPU all-pairs engine (gtsfm_amd/frontend/all_pairs.py with HipKernels) and the compaction kernel
(gtsfm_compact_verified) against the oracle.

- compaction: random masks / statuses / ragged putative counts (mcap not a multiple of 64, empty pairs, failed
  pairs) vs a numpy restatement of `match_indices[mask == 1]` (opencv_verifier_base.py:98-100) and the inlier-support
  filter (inlier_support_processor.py:73-87): bit-exact;
- the engine, host images in -> host results out, with image and pair chunking, vs the same engine driven by the
  oracle kernels on CPU: keypoints and putative counts bit-exact, statuses equal, inlier counts equal, R/t
  bit-identical and the same verified rows (the verifier's bar in tests/test_verifier_gpu.py);
- device-resident steps leave the same results on the device as host steps.
"""
import dataclasses

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


def _compact_ref(idx, cnt, mask, status, n_inl, min_inl, min_ratio, ratio_inliers=None):
    """ratio_inliers: the counts the inlier ratio is taken on (the pre-BA ones after BA); rows, offsets and the
    min-inlier guard stay on n_inl."""
    rows, off, ok = [], [0], []
    for p in range(len(cnt)):
        M, st, n = int(cnt[p]), int(status[p]), int(n_inl[p])
        nr = n if ratio_inliers is None else int(ratio_inliers[p])
        ratio = nr / M if (st == 0 and M > 0) else 0.0
        ok.append(int(st == 0 and not (ratio < min_ratio or (0 < n < min_inl))))
        r = idx[p, :M][mask[p, :M].astype(bool)] if st == 0 else np.zeros((0, 2), np.int32)
        rows.append(r)
        off.append(off[-1] + len(r))
    return np.array(off), np.concatenate(rows) if rows else np.zeros((0, 2)), np.array(ok)


# P = 1024, 1025 and 2500: the scan's threads take one pair each with none idle, two each with half of them idle, and
# three each with a ragged last thread
@pytest.mark.parametrize("P,mcap", [(1, 7), (37, 130), (300, 64), (1000, 513), (1024, 9), (1025, 9), (2500, 70)])
def test_compact_verified_matches_restatement(dev, P, mcap):
    from gtsfm_amd import device

    rng = np.random.default_rng(P * 1000 + mcap)
    idx = rng.integers(0, 5000, size=(P, mcap, 2)).astype(np.int32)
    cnt = rng.integers(0, mcap + 1, size=P).astype(np.int32)
    cnt[: min(3, P)] = [0, mcap, 5][: min(3, P)]
    mask = (rng.random((P, mcap)) < rng.random((P, 1))).astype(np.uint8)
    mask[np.arange(mcap)[None, :] >= cnt[:, None]] = rng.integers(0, 2)  # junk past the putatives is ignored
    n_inl = np.array([int(mask[p, : cnt[p]].sum()) for p in range(P)], np.int32)
    status = rng.choice([0, 0, 0, 1, 2], size=P).astype(np.int32)
    status[cnt < 6] = 1
    n_inl[status != 0] = 0

    class Res:
        pass

    res = Res()
    res.mask = torch.from_numpy(mask).to(dev)
    res.status = torch.from_numpy(status).to(dev)
    res.n_inliers = torch.from_numpy(n_inl).to(dev)
    cap = int(cnt.sum())
    off, rows, ok = device.compact_verified(torch.from_numpy(idx).to(dev), torch.from_numpy(cnt).to(dev), res, 15, 0.1,
                                            cap)
    e_off, e_rows, e_ok = _compact_ref(idx, cnt, mask, status, n_inl, 15, 0.1)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(off.cpu().numpy(), e_off)
    np.testing.assert_array_equal(rows.cpu().numpy()[: e_off[-1]], e_rows.reshape(-1, 2))
    np.testing.assert_array_equal(ok.cpu().numpy()[:P], e_ok)


class _Res:
    """The verifier outputs gtsfm_compact_verified consumes."""

    def __init__(self, dev, mask, status, n_inl):
        self.mask = torch.from_numpy(np.ascontiguousarray(mask, np.uint8)).to(dev)
        self.status = torch.from_numpy(np.ascontiguousarray(status, np.int32)).to(dev)
        self.n_inliers = torch.from_numpy(np.ascontiguousarray(n_inl, np.int32)).to(dev)


def _random_compact_case(rng, P, mcap):
    idx = rng.integers(0, 5000, size=(P, mcap, 2)).astype(np.int32)
    cnt = rng.integers(0, mcap + 1, size=P).astype(np.int32)
    mask = (rng.random((P, mcap)) < rng.random((P, 1))).astype(np.uint8)
    mask[np.arange(mcap)[None, :] >= cnt[:, None]] = 1  # junk past the putatives is ignored
    n_inl = np.array([int(mask[p, : cnt[p]].sum()) for p in range(P)], np.int32)
    status = rng.choice([0, 0, 0, 1, 2], size=P).astype(np.int32)
    status[cnt < 6] = 1
    n_inl[status != 0] = 0
    return idx, cnt, mask, status, n_inl


def test_compact_ratio_inliers_decide_the_ratio_only(dev):
    """d_ratio_inliers (the pre-BA counts): isp_ok follows ratio_inliers / M, offsets and rows follow n_inliers."""
    from gtsfm_amd import device

    rng = np.random.default_rng(77)
    P, mcap = 200, 200
    idx, cnt, mask, status, n_inl = _random_compact_case(rng, P, mcap)
    ratio_inl = rng.integers(0, cnt + 1).astype(np.int32)  # unrelated to n_inl, within [0, M]
    ratio_inl[status != 0] = 0
    e_off, e_rows, e_ok = _compact_ref(idx, cnt, mask, status, n_inl, 15, 0.3, ratio_inliers=ratio_inl)
    _, _, plain_ok = _compact_ref(idx, cnt, mask, status, n_inl, 15, 0.3)
    assert np.count_nonzero(ratio_inl != n_inl) > P // 2
    assert np.count_nonzero((e_ok == 1) & (plain_ok == 0)) >= 3 and np.count_nonzero((e_ok == 0) & (plain_ok == 1)) >= 3
    off, rows, ok = device.compact_verified(torch.from_numpy(idx).to(dev), torch.from_numpy(cnt).to(dev),
                                            _Res(dev, mask, status, n_inl), 15, 0.3, int(cnt.sum()),
                                            ratio_inliers=torch.from_numpy(ratio_inl).to(dev))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(off.cpu().numpy(), e_off)
    np.testing.assert_array_equal(rows.cpu().numpy()[: e_off[-1]], e_rows.reshape(-1, 2))
    np.testing.assert_array_equal(ok.cpu().numpy()[:P], e_ok)


@pytest.mark.parametrize("min_ratio", [0.1, 0.0])
def test_compact_inlier_support_boundaries(dev, min_ratio):
    """inlier_support_processor.py:73-87 on its boundaries, min_inliers = 5: failure iff ratio < min_ratio or
    0 < n < min_inliers, so a ratio exactly at min_ratio and a count exactly at min_inliers pass."""
    from gtsfm_amd import device

    #        (n, M): 5/50 = ratio 0.1 exactly and n == min_inliers; 4/40 = 0.1 but n == min_inliers - 1; 5/20 and
    #        4/20 the same two counts well above the ratio; 0/30 no inliers with status 0; 5/51 just below 0.1
    cases = [(5, 50), (4, 40), (5, 20), (4, 20), (0, 30), (5, 51)]
    expect = {0.1: [1, 0, 1, 0, 0, 0], 0.0: [1, 0, 1, 0, 1, 1]}[min_ratio]
    P, mcap = len(cases), 64
    rng = np.random.default_rng(5)
    idx = rng.integers(0, 5000, size=(P, mcap, 2)).astype(np.int32)
    cnt = np.array([M for _, M in cases], np.int32)
    n_inl = np.array([n for n, _ in cases], np.int32)
    mask = np.zeros((P, mcap), np.uint8)
    for p, (n, M) in enumerate(cases):
        mask[p, rng.choice(M, n, replace=False)] = 1
    status = np.zeros(P, np.int32)
    e_off, e_rows, e_ok = _compact_ref(idx, cnt, mask, status, n_inl, 5, min_ratio)
    assert e_ok.tolist() == expect
    off, rows, ok = device.compact_verified(torch.from_numpy(idx).to(dev), torch.from_numpy(cnt).to(dev),
                                            _Res(dev, mask, status, n_inl), 5, min_ratio, int(n_inl.sum()))
    torch.cuda.synchronize()
    assert ok.cpu().numpy()[:P].tolist() == expect
    np.testing.assert_array_equal(off.cpu().numpy(), e_off)
    np.testing.assert_array_equal(rows.cpu().numpy()[: e_off[-1]], e_rows.reshape(-1, 2))


def test_compact_capacity_below_the_total(dev):
    """A v_corr buffer shorter than the total: offsets are still the full scan, every pair that fits has its rows,
    and nothing at or past `capacity` rows is written."""
    from gtsfm_amd import device

    rng = np.random.default_rng(78)
    P, mcap = 60, 40
    idx, cnt, mask, status, n_inl = _random_compact_case(rng, P, mcap)
    e_off, e_rows, e_ok = _compact_ref(idx, cnt, mask, status, n_inl, 15, 0.1)
    total = int(e_off[-1])
    capacity = total // 2
    fits = [p for p in range(P) if status[p] == 0 and e_off[p] + n_inl[p] <= capacity]
    assert 0 < len(fits) and any(status[p] == 0 and n_inl[p] > 0 and e_off[p] + n_inl[p] > capacity for p in range(P))
    big = torch.full((total + 16, 2), -7, dtype=torch.int32, device=dev)
    off, rows, ok = device.compact_verified(torch.from_numpy(idx).to(dev), torch.from_numpy(cnt).to(dev),
                                            _Res(dev, mask, status, n_inl), 15, 0.1, capacity,
                                            out_v_corr=big[:capacity])
    torch.cuda.synchronize()
    np.testing.assert_array_equal(off.cpu().numpy(), e_off)
    np.testing.assert_array_equal(ok.cpu().numpy()[:P], e_ok)
    got = big.cpu().numpy()
    for p in fits:
        np.testing.assert_array_equal(got[e_off[p]: e_off[p + 1]], e_rows.reshape(-1, 2)[e_off[p]: e_off[p + 1]])
    assert (got[capacity:] == -7).all()


def _engine(kernels, device, n_img, scene, world=1, rank=0):
    from gtsfm_amd.frontend import sharding
    from gtsfm_amd.frontend.all_pairs import AllPairsFrontEnd, FrontEndConfig

    mine = sharding.local_images(n_img, world, rank)
    cfg = FrontEndConfig(kpts=600, extract_chunk=3, pair_chunk=5)
    return AllPairsFrontEnd(scene.images[mine].cpu(), scene.intrinsics[:n_img], n_img, rank, world, device, cfg,
                            kernels=kernels)


def test_engine_host_to_host_matches_oracle_engine(dev):
    from gtsfm_amd import synthetic
    from oracle_kernels import OracleKernels

    n_img = 7
    scene = synthetic.render_scene(24, 360, 480, device="cuda", indices=range(n_img))
    gpu = _engine(None, dev, n_img, scene)
    ref_fe = _engine(OracleKernels(), torch.device("cpu"), n_img, scene)
    def own(r):  # HostResults views pinned buffers that the next step overwrites
        return dataclasses.replace(r, **{f.name: np.array(getattr(r, f.name)) for f in dataclasses.fields(r)})

    got = own(gpu.step())
    got_again = own(gpu.step())  # a second step into the same pinned buffers reproduces the first
    ref = ref_fe.step()
    np.testing.assert_array_equal(got.kp_count, ref.kp_count)
    for i in range(n_img):
        np.testing.assert_array_equal(got.kp_xy[i, : got.kp_count[i]], ref.kp_xy[i, : ref.kp_count[i]])
    np.testing.assert_array_equal(got.n_matches, ref.n_matches)
    np.testing.assert_array_equal(got.status, ref.status)
    assert (got.status == 0).sum() >= 10
    for p in range(len(got.pairs)):
        if got.status[p] != 0:
            assert len(got.verified(p)) == 0
            continue
        n, rn = int(got.n_inliers[p]), int(ref.n_inliers[p])
        assert n == rn, (p, n, rn)
        assert len(got.verified(p)) == n
        np.testing.assert_array_equal(got.R[p], ref.R[p])
        np.testing.assert_array_equal(got.t[p], ref.t[p])
        np.testing.assert_array_equal(got.verified(p), ref.verified(p))
        assert got.isp_ok[p] == ref.isp_ok[p]
    np.testing.assert_array_equal(got_again.v_corr, got.v_corr)
    np.testing.assert_array_equal(got_again.offsets, got.offsets)
    # a resident step recomputes the same device results
    before = gpu.d_v_corr.clone()
    gpu.step(resident=True)
    torch.cuda.synchronize()
    assert torch.equal(gpu.d_v_corr, before)


def test_engine_with_two_view_bundle_adjustment(dev):
    """bundle_adjust_2view=True (every shipped config): RANSAC -> two-view triangulation + BA -> compaction + ISP on
    the post-BA rows with the pre-BA inlier ratio, against the same engine on the oracle kernels (RANSAC masks differ
    within 1 %, so BA sees slightly different rows: counts within 2 % + 2, poses within 0.1 deg)."""
    from gtsfm_amd import synthetic
    from gtsfm_amd.frontend import sharding
    from gtsfm_amd.frontend.all_pairs import AllPairsFrontEnd, FrontEndConfig
    from oracle_kernels import OracleKernels

    n_img = 5
    scene = synthetic.render_scene(24, 360, 480, device="cuda", indices=range(n_img))
    cfg = FrontEndConfig(kpts=600, extract_chunk=3, pair_chunk=4, bundle_adjust=True)
    mine = sharding.local_images(n_img, 1, 0)
    host = scene.images[mine].cpu()
    gpu = AllPairsFrontEnd(host, scene.intrinsics[:n_img], n_img, 0, 1, dev, cfg).step()
    ref = AllPairsFrontEnd(host, scene.intrinsics[:n_img], n_img, 0, 1, torch.device("cpu"), cfg,
                           kernels=OracleKernels()).step()
    np.testing.assert_array_equal(gpu.status, ref.status)
    ran = 0
    for p in range(len(gpu.pairs)):
        if gpu.status[p] != 0:
            continue
        n, rn = int(gpu.n_inliers[p]), int(ref.n_inliers[p])
        assert abs(n - rn) <= 0.02 * rn + 2, (p, n, rn)
        assert len(gpu.verified(p)) == n
        assert scenes.rotation_angle_deg(gpu.R[p], ref.R[p]) < 0.1
        ran += int(n > 0)
    assert ran >= 4
