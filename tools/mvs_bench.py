#!/usr/bin/env python
"""Times the dense-MVS geometry stages (view selection, depth fusion, point gathering, voxel size and downsampling) on
an analytic scene of C4-like shape.

Scene: --images cameras on an arc in front of the plane z = 10 with a sphere of radius 1.5 before it, all looking at the
sphere; depth maps of --height x --width are rendered analytically on the device (ray against plane and sphere, plain
torch: data generation, not timed), 5 % of the pixels get a wrong depth and the confidence is uniform in [0.6, 1];
--tracks surface points are each seen by a run of 2-5 neighbouring cameras. Every stage is timed with the
tools' shared helper (tracks_bench.time_launches: warm-up, then --repeats windows of at least 100 ms between events);
the median per launch is reported in milliseconds, with the points in and out. The two
stages that read a count on the host (the point count, the voxel count) include that synchronisation.

With --restatement (use a small shape) every output must agree with tests/mvs_ref.py on the same input, and the
restatement's own time is reported as the baseline. The reference's host path (cv2.remap, Open3D) is not available to
run here, so no other comparison is made.

    python tools/mvs_bench.py [--images 1000 --height 1080 --width 1920] [--out bench_out/mvs.jsonl]
    python tools/mvs_bench.py --images 8 --height 96 --width 128 --tracks 400 --restatement
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tracks_bench import time_launches  # noqa: E402  (the tools' shared timing helper)

from gtsfm_amd import device, native  # noqa: E402
from gtsfm_amd.densify import mvs_utils  # noqa: E402
from gtsfm_amd.densify.mvs_depth_fusion import fuse_depth_arrays, select_views_arrays  # noqa: E402
from tests.mvs_ref import PLANE_Z, SPHERE_C, SPHERE_R, look_at  # noqa: E402  (the scene of the MVS tests)


def render_depth(wRc, wtc, intr, H, W, dev):
    """tests/mvs_ref.render_depth in torch on the device: (n, H, W) float32 z-depth of the plane and the sphere at the
    integer pixel coordinates (1000 maps of 1080p are not rendered on the host)."""
    n = len(wtc)
    out = torch.empty((n, H, W), dtype=torch.float32, device=dev)
    y, x = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64),
                          torch.arange(W, device=dev, dtype=torch.float64), indexing="ij")
    R_all, t_all, K_all = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (wRc, wtc, intr))
    centre = torch.from_numpy(SPHERE_C).to(dev)
    for i in range(n):
        R, o, K = R_all[i], t_all[i], K_all[i]
        rays = torch.stack([(x - K[1]) / K[0], (y - K[2]) / K[0], torch.ones_like(x)], -1) @ R.T
        t_plane = (PLANE_Z - o[2]) / rays[..., 2]
        oc = o - centre
        a = (rays * rays).sum(-1)
        b = 2.0 * (rays @ oc)
        disc = b * b - 4.0 * a * (oc @ oc - SPHERE_R ** 2)
        t_sphere = torch.where(disc > 0, (-b - disc.clamp_min(0).sqrt()) / (2.0 * a), torch.full_like(a, float("inf")))
        t_sphere = torch.where(t_sphere > 0, t_sphere, torch.full_like(a, float("inf")))
        out[i] = torch.minimum(t_plane, t_sphere).to(torch.float32)
    return out


def make_scene(n_img, H, W, n_tracks, seed, dev):
    rng = np.random.default_rng(seed)
    ang = np.linspace(-0.5, 0.5, n_img)
    wtc = np.stack([6.0 * np.sin(ang), 0.3 * np.cos(3 * ang), 7.0 - 7.0 * np.cos(ang)], 1)
    wRc = np.stack([look_at(c, SPHERE_C + rng.normal(0, 0.05, 3)) for c in wtc])
    intr = np.tile(np.array([1.1 * W, (W - 1) / 2.0, (H - 1) / 2.0]), (n_img, 1))
    lens = rng.integers(2, 6, n_tracks)
    start = rng.integers(0, max(n_img - 5, 1), n_tracks)
    img = np.concatenate([np.minimum(s + np.arange(k), n_img - 1) for s, k in zip(start, lens)]).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    point = np.stack([rng.uniform(-3, 3, n_tracks), rng.uniform(-2, 2, n_tracks), np.full(n_tracks, PLANE_Z)], 1)
    depth = render_depth(wRc, wtc, intr, H, W, dev)
    g = torch.Generator(device=dev).manual_seed(seed)
    wrong = torch.rand(depth.shape, generator=g, device=dev) < 0.05
    depth = torch.where(wrong, depth * (0.5 + torch.rand(depth.shape, generator=g, device=dev)), depth).contiguous()
    conf = (0.6 + 0.4 * torch.rand(depth.shape, generator=g, device=dev)).contiguous()
    images = torch.randint(0, 256, (n_img, H, W, 3), generator=g, device=dev, dtype=torch.uint8)
    return dict(wRc=wRc, wtc=wtc, intr=intr, offsets=offsets, img=img, point=point, depth=depth, conf=conf,
                images=images)


class Csr:
    def __init__(self, offsets, image):
        self.offsets, self.image = offsets, image


WARMUP, WINDOW_MS = 2, 100.0


def timed(fn, repeats):
    """Median milliseconds per launch of fn (time_launches: warm-up, then `repeats` windows of at least WINDOW_MS), and
    fn's result."""
    out = fn()
    _, ms = time_launches(fn, WARMUP, repeats, WINDOW_MS)
    return statistics.median(ms), out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--tracks", type=int, default=200000)
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--restatement", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    native.require_gpu()
    dev = torch.device("cuda")
    s = make_scene(a.images, a.height, a.width, a.tracks, a.seed, dev)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    cams = (up(s["wRc"]), up(s["wtc"]), up(s["intr"]), None)
    tracks, point = Csr(up(s["offsets"]), up(s["img"])), up(s["point"])
    ms = {}
    ms["select_views"], views = timed(lambda: select_views_arrays(cams, tracks, point, None, None, a.views), a.repeats)
    ms["fuse_and_gather"], dense = timed(lambda: fuse_depth_arrays(s["depth"], s["conf"], s["images"], cams, views),
                                         a.repeats)
    wRc, wtc, intr = cams[:3]
    ms["fuse_depth_kernels"], _ = timed(lambda: device.mvs_fuse_depth(s["depth"], s["conf"], wRc, wtc, intr,
                                                                      views.src_views), a.repeats)
    ms["voxel_size"], (voxel, stats) = timed(lambda: mvs_utils.estimate_minimum_voxel_size_arrays(dense.points),
                                             a.repeats)
    ms["voxel_downsample"], (p_down, c_down) = timed(
        lambda: mvs_utils.downsample_point_cloud_arrays(dense.points, dense.colors, voxel, stats), a.repeats)
    line = {"tool": "mvs_bench", "images": a.images, "height": a.height, "width": a.width, "tracks": a.tracks,
            "sources": int(views.src_views.shape[1]), "points": int(dense.points.shape[0]),
            "points_downsampled": int(p_down.shape[0]), "voxel_size": voxel,
            "ms": {k: round(v, 3) for k, v in ms.items()},
            "pixel_source_pairs_per_s": a.images * a.height * a.width * int(views.src_views.shape[1])
            / (ms["fuse_depth_kernels"] * 1e-3)}
    if a.restatement:
        from tests import mvs_ref as M

        t0 = time.perf_counter()
        v = M.select_views(s["offsets"], s["img"], s["point"], None, None, s["wRc"], s["wtc"], None, a.views)
        depth, conf, images = (x.cpu().numpy() for x in (s["depth"], s["conf"], s["images"]))
        f = M.fuse_depth(depth, conf, s["wRc"], s["wtc"], s["intr"], v.src_views)
        pts, cols, off = M.gather_points(f.fused, f.mask, s["wRc"], s["wtc"], s["intr"], images)
        st = M.voxel_stats(pts)
        vox = M.voxel_size(st, len(pts))
        w_p, w_c, _, _ = M.voxel_downsample(pts, cols, st[12:15], vox)
        line["restatement_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        assert np.all(np.abs(views.scores_fixed.cpu().numpy() - v.scores) <= v.terms)
        np.testing.assert_array_equal(views.src_views.cpu().numpy(), v.src_views)
        np.testing.assert_allclose(views.depth_range.cpu().numpy(), v.depth_range, rtol=1e-12)
        differ = dense.mask.cpu().numpy() != f.mask
        line["mask_pixels_that_differ"] = int(differ.sum())
        assert differ.mean() <= 0.01
        if not differ.any():
            np.testing.assert_allclose(dense.points.cpu().numpy(), pts, rtol=0, atol=1e-9)
            np.testing.assert_array_equal(dense.colors.cpu().numpy(), cols)
            assert voxel == float(np.float64(vox)) or abs(voxel - vox) <= 1e-9 * vox
            assert p_down.shape[0] == len(w_p)
            np.testing.assert_allclose(p_down.cpu().numpy(), w_p, rtol=0, atol=1e-9)
        line["restatement_agrees"] = True
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
