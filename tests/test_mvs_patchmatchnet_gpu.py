"""The dense-MVS stage with the HIP PatchmatchNet as its depth estimator, on tests/test_mvs_chain_gpu.py's scene (its
cached MultiViewOptimizer result): MVSDepthFusion(PatchmatchNetDepthEstimator) and MVSPatchmatchNet.densify give the
cloud that fusing the maps of a direct gtsfm_patchmatchnet_batched call gives. The weights are random, so the
confidence is near 0.5 and the geometric checks are loosened until points survive; what the cloud looks like is not the
subject here."""
import numpy as np
import pytest
import torch

from patchmatchnet_weights import patchmatchnet_state_dict
from tests import test_mvs_chain_gpu as chain

pytestmark = pytest.mark.gpu

THRESHOLDS = dict(max_geo_pixel_thresh=4.0, max_geo_depth_thresh=0.5, min_conf_thresh=0.3, min_num_consistent_views=1)
SEED = 3


@pytest.fixture(scope="module")
def blob():
    from gtsfm_amd.densify import pack_patchmatchnet_weights

    return pack_patchmatchnet_weights(patchmatchnet_state_dict(0))


def test_depth_fusion_with_the_patchmatchnet_estimator(blob):
    from gtsfm_amd import device
    from gtsfm_amd.densify import PatchmatchNetDepthEstimator
    from gtsfm_amd.densify import mvs_depth_fusion as mdf

    sc, _ = chain._scene()
    r = chain._run_arrays()
    estimator = PatchmatchNetDepthEstimator(blob, seed=SEED)
    dense, views = mdf.MVSDepthFusion(estimator, **THRESHOLDS).densify_arrays(sc.images, r)
    nv = views.pm_to_img.numel()
    assert dense.fused.shape == (nv, chain.H, chain.W) and nv >= 8

    cameras = (r.ba.wRc, r.ba.wtc, r.cameras[2], r.ba.cam_keep)
    wRc, wtc, intr = mdf.valid_cameras(cameras, views)
    crop = sc.images[views.pm_to_img.long(), : chain.H, : chain.W].contiguous()
    direct = device.patchmatchnet_depth(crop, wRc, wtc, intr, views.src_views, views.depth_range, chain._t(blob),
                                        estimator.init_uniform(nv, chain.H, chain.W, crop.device))
    assert direct.depth.shape == (nv, chain.H, chain.W) and direct.confidence.shape == (nv, chain.H, chain.W)
    assert torch.isfinite(direct.depth).all() and torch.isfinite(direct.confidence).all()
    lo, hi = views.depth_range[:, 0].min().item(), views.depth_range[:, 1].max().item()
    print("views", nv, "depth", direct.depth.min().item(), direct.depth.max().item(), "range", lo, hi, "confidence",
          direct.confidence.min().item(), direct.confidence.max().item(), "points", len(dense.points))
    want = mdf.fuse_depth_arrays(direct.depth, direct.confidence, sc.images, cameras, views, *THRESHOLDS.values())
    assert len(want.points) > 0
    assert torch.equal(dense.points, want.points) and torch.equal(dense.colors, want.colors)
    assert torch.equal(dense.fused, want.fused)


def test_mvs_patchmatchnet_densify_has_the_reference_signature(blob):
    from gtsfm_amd.bundle.bundle_adjustment import BaData
    from gtsfm_amd.common import geometry as g
    from gtsfm_amd.common.image import Image
    from gtsfm_amd.common.sfm_track import SfmTrack
    from gtsfm_amd.densify import MVSPatchmatchNet, PatchmatchNetDepthEstimator
    from gtsfm_amd.densify import mvs_depth_fusion as mdf

    sc, _ = chain._scene()
    r = chain._run_arrays()
    dense, _ = mdf.MVSDepthFusion(PatchmatchNetDepthEstimator(blob, seed=SEED), **THRESHOLDS).densify_arrays(sc.images, r)
    n = chain.N_IMG
    wRc, wtc = r.ba.wRc.cpu().numpy().reshape(n, 3, 3), r.ba.wtc.cpu().numpy().reshape(n, 3)
    intr, keep = r.cameras[2].cpu().numpy().reshape(n, 3), r.ba.cam_keep.cpu().numpy()
    cams = {int(i): g.PinholeCameraCal3Bundler(g.Pose3(g.Rot3(wRc[i]), wtc[i]),
                                               g.Cal3Bundler(intr[i, 0], 0, 0, intr[i, 1], intr[i, 2]))
            for i in np.flatnonzero(keep)}
    offsets, img = r.tracks.offsets.cpu().numpy(), r.tracks.image.cpu().numpy()
    point, track_keep = r.ba.point.cpu().numpy().reshape(-1, 3), r.ba.track_keep.cpu().numpy()
    inlier = r.triangulated.inlier.cpu().numpy()
    tracks = []
    for t in np.flatnonzero(track_keep):
        track = SfmTrack(point[t])
        for m in range(offsets[t], offsets[t + 1]):
            if inlier[m] and keep[img[m]]:
                track.addMeasurement(int(img[m]), np.zeros(2))
        tracks.append(track)
    images = {i: Image(sc.images[i].cpu().numpy()) for i in range(n)}
    points, colors, metrics = MVSPatchmatchNet(weights=blob, seed=SEED).densify(images, BaData(cams, tracks), **THRESHOLDS)
    np.testing.assert_array_equal(points, dense.points.cpu().numpy())
    np.testing.assert_array_equal(colors, dense.colors.cpu().numpy())
    assert len(metrics["joint_mask_valid_ratios"]) == len(cams)
    with pytest.raises(ValueError):
        MVSPatchmatchNet(weights=blob).densify(images, BaData(cams, tracks), num_workers=2)
