#!/usr/bin/env python
"""Times the back-end chain (MultiViewOptimizer.run_arrays) stage by stage and as a whole on a synthetic scene.

Scene: --images cameras on a ring of radius 10 looking at the origin, --tracks points in a ball of radius 2, each seen
by a run of 10-19 neighbouring cameras (about 14.5 measurements per track, the C4 shape of tools/global_ba_bench.py and
tools/tracks_bench.py); every two cameras at most 18 apart on the ring are a pair with the exact relative pose, and its
verified correspondences are the points both see. Keypoints are exact projections rounded to float32. The stages
synchronise their streams, so each is timed with a host clock around it, after one warm-up run of the whole chain;
gtsfm_assemble_ba_input alone is timed with events over --repeats launches. Reported: milliseconds per stage, their
sum, the whole run_arrays call, and the assemble call. With --restatement the assemble outputs must equal
tests/multi_view_ref.assemble_ref on the same input, and that restatement is timed.

    python tools/multi_view_bench.py [--images 1000] --restatement [--out bench_out/multi_view.jsonl]
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

from gtsfm_amd import device, native  # noqa: E402
from gtsfm_amd.averaging.rotation.shonan import ShonanRotationAveraging  # noqa: E402
from gtsfm_amd.averaging.translation.averaging_1dsfm import TranslationAveraging1DSFM  # noqa: E402
from gtsfm_amd.bundle.bundle_adjustment import BundleAdjustmentOptimizer  # noqa: E402
from gtsfm_amd.data_association.data_assoc import DataAssociation  # noqa: E402
from gtsfm_amd.data_association.dsf_tracks_estimator import DsfTracksEstimator  # noqa: E402
from gtsfm_amd.data_association.point3d_initializer import TriangulationOptions, TriangulationSamplingMode  # noqa: E402
from gtsfm_amd.multi_view_optimizer import MultiViewOptimizer, init_cameras_arrays  # noqa: E402
from gtsfm_amd.view_graph_estimator.cycle_consistent_rotation_estimator import (  # noqa: E402
    CycleConsistentRotationViewGraphEstimator,
    EdgeErrorAggregationCriterion,
)

MAX_GAP = 18  # two cameras of one track are at most this far apart on the ring


def ring_scene(n_img: int, n_pts: int, seed: int) -> dict:
    rng = np.random.default_rng(seed)
    ang = 2 * np.pi * np.arange(n_img) / n_img
    eyes = np.stack([10 * np.cos(ang), 10 * np.sin(ang), rng.uniform(-2.0, 2.0, n_img)], 1)
    z = -eyes / np.linalg.norm(eyes, axis=1, keepdims=True)
    x = np.cross(np.array([0.0, 0.0, -1.0]), z)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    wRc = np.stack([x, np.cross(z, x), z], axis=2)
    intr = np.tile(np.array([800.0, 500.0, 400.0]), (n_img, 1))
    pts = rng.uniform(-2.0, 2.0, (n_pts, 3))
    lens = rng.integers(10, MAX_GAP + 2, n_pts)
    start = rng.integers(0, n_img, n_pts)
    cam = np.concatenate([(s + np.arange(k)) % n_img for s, k in zip(start, lens)])
    pt = np.repeat(np.arange(n_pts), lens)
    order = np.lexsort((pt, cam))  # keypoints of an image in point order
    kp = np.empty(len(cam), np.int64)
    first = np.searchsorted(cam[order], np.arange(n_img))
    kp[order] = np.arange(len(cam)) - first[cam[order]]
    kp_count = np.bincount(cam, minlength=n_img).astype(np.int32)
    kmax = int(kp_count.max())
    pc = np.einsum("nji,nj->ni", wRc[cam], pts[pt] - eyes[cam])
    kp_xy = np.zeros((n_img, kmax, 2), np.float32)
    kp_xy[cam, kp] = intr[cam, 1:3] + intr[cam, :1] * pc[:, :2] / pc[:, 2:3]
    off = np.concatenate([[0], np.cumsum(lens)])
    c1, c2, k1, k2 = [], [], [], []
    for L in np.unique(lens):
        sel = np.flatnonzero(lens == L)
        a, b = np.triu_indices(L, 1)
        base = off[sel][:, None]
        c1.append(cam[base + a].ravel()), c2.append(cam[base + b].ravel())
        k1.append(kp[base + a].ravel()), k2.append(kp[base + b].ravel())
    c1, c2, k1, k2 = (np.concatenate(v) for v in (c1, c2, k1, k2))
    swap = c1 > c2
    c1, c2, k1, k2 = np.where(swap, c2, c1), np.where(swap, c1, c2), np.where(swap, k2, k1), np.where(swap, k1, k2)
    key = c1 * n_img + c2
    order = np.argsort(key, kind="stable")
    ukey, counts = np.unique(key[order], return_counts=True)
    pairs = np.stack([ukey // n_img, ukey % n_img], 1).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    v_corr = np.stack([k1[order], k2[order]], 1).astype(np.int32)
    i1, i2 = pairs[:, 0], pairs[:, 1]
    i2Ri1 = np.einsum("nji,njk->nik", wRc[i2], wRc[i1])
    i2Ui1 = np.einsum("nji,nj->ni", wRc[i2], eyes[i1] - eyes[i2])
    i2Ui1 /= np.linalg.norm(i2Ui1, axis=1, keepdims=True)
    return dict(pairs=pairs, i2Ri1=i2Ri1, i2Ui1=i2Ui1, pair_valid=np.ones(len(pairs), np.uint8), offsets=offsets,
                v_corr=v_corr, kp_count=kp_count, kmax=kmax, kp_xy=kp_xy, intrinsics=intr, num_images=n_img)


ARGS = ("pairs", "i2Ri1", "i2Ui1", "pair_valid", "offsets", "v_corr", "kp_count", "kmax", "kp_xy", "intrinsics",
        "num_images")


class Clock:
    def __init__(self):
        self.ms = {}

    def __call__(self, name, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        self.ms[name] = (time.perf_counter() - t0) * 1e3
        return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--tracks", type=int, default=14000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--restatement", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    native.require_gpu()
    dev = torch.device("cuda:0")
    s = ring_scene(a.images, a.tracks, a.seed)
    d = [s[k] if k in ("kmax", "num_images") else torch.from_numpy(np.ascontiguousarray(s[k])).to(dev) for k in ARGS]
    pairs, i2Ri1, i2Ui1, pair_valid, offsets, v_corr, kp_count, kmax, kp_xy, intr, n = d
    vg = CycleConsistentRotationViewGraphEstimator(EdgeErrorAggregationCriterion.MEDIAN_EDGE_ERROR)
    rot_m, trans_m = ShonanRotationAveraging(), TranslationAveraging1DSFM()
    da = DataAssociation(3, TriangulationOptions(TriangulationSamplingMode.NO_RANSAC, 3.0))
    ba_m = BundleAdjustmentOptimizer(reproj_error_thresholds=[3.0], robust_measurement_noise=True)
    opt = MultiViewOptimizer(rot_m, trans_m, da, ba_m, vg)
    clock = Clock()
    clock("warm_up", lambda: opt.run_arrays(*d))
    whole = clock("run_arrays", lambda: opt.run_arrays(*d))
    assert whole.ba is not None, "the chain stopped early"

    keep = clock("view_graph", lambda: vg.run_arrays(pairs, i2Ri1, valid=pair_valid, num_images=n))[0].to(torch.uint8)
    rot = clock("rotation_averaging", lambda: rot_m.run_rotation_averaging_arrays(pairs, i2Ri1, keep, n))
    tracks = clock("tracks", lambda: DsfTracksEstimator().run_arrays(pairs, offsets, v_corr, kp_count, kmax,
                                                                      valid=keep, kp_xy=kp_xy))
    trans = clock("translation_averaging", lambda: trans_m.run_translation_averaging_arrays(
        pairs, i2Ui1, rot.wRi, edge_valid=keep, rot_valid=rot.rot_valid, track_offsets=tracks.offsets,
        track_img=tracks.image, track_uv=tracks.uv, intrinsics=intr))
    cams = clock("init_cameras", lambda: init_cameras_arrays(rot.wRi, trans.wti, trans.wti_valid, intr))
    tri, valid = clock("triangulation", lambda: da.run_triangulation_arrays(cams, tracks))
    ba_in = clock("assemble", lambda: da.assemble_arrays(tracks, tri, valid, cams[3]))
    ba = clock("bundle_adjustment", lambda: ba_m.run_ba_arrays((cams[0], cams[1], cams[2], ba_in.cam_keep), tracks, tri,
                                                               ba_in.track_keep, reproj_error_thresh=3.0))
    for x, y in ((whole.ba_input.cam_keep, ba_in.cam_keep), (whole.ba_input.track_keep, ba_in.track_keep),
                 (whole.ba.wRc, ba.wRc), (whole.ba.wtc, ba.wtc), (whole.ba.stats, ba.stats)):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), "run_arrays differs from the stages by hand"

    # the assemble call alone, between events
    T = tri.exit_code.numel()
    valid_u8, inl = valid.to(torch.uint8).contiguous(), tri.inlier.contiguous()
    ws = torch.empty(max(native.lib().gtsfm_assemble_ba_input_workspace_bytes(T, n), 256), dtype=torch.uint8, device=dev)
    call = lambda: device.assemble_ba_input(tracks.offsets, tracks.image, valid_u8, inl, cams[3], n, n_tracks=T,  # noqa
                                            workspace=ws)
    call()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.repeats)]
    for e0, e1 in ev:
        e0.record()
        last = call()
        e1.record()
    torch.cuda.synchronize()
    kernel_ms = [e0.elapsed_time(e1) for e0, e1 in ev]
    stages = ("view_graph", "rotation_averaging", "tracks", "translation_averaging", "init_cameras", "triangulation",
              "assemble", "bundle_adjustment")
    res = {"tool": "multi_view_bench", "images": n, "pairs": int(pairs.shape[0]), "rows": int(v_corr.shape[0]),
           "tracks": int(T), "measurements": int(tracks.image.numel()),
           "stage_ms": {k: clock.ms[k] for k in stages}, "stages_sum_ms": sum(clock.ms[k] for k in stages),
           "run_arrays_ms": clock.ms["run_arrays"], "warm_up_ms": clock.ms["warm_up"],
           "assemble_call_ms_median": statistics.median(kernel_ms), "assemble_call_ms_min": min(kernel_ms),
           "assemble_stats": dict(zip(native.BA_INPUT_STATS_FIELDS, last.stats.cpu().tolist())),
           "ba_stats": dict(zip(native.GBA_STATS_FIELDS, ba.stats.cpu().tolist()))}
    if a.restatement:
        from tests import multi_view_ref

        host = [t.cpu().numpy() for t in (tracks.offsets, tracks.image, valid_u8, inl, cams[3])]
        t0 = time.perf_counter()
        want = multi_view_ref.assemble_ref(*host, n)
        res["restatement_s"] = time.perf_counter() - t0
        for k in ("cam_keep", "track_keep", "track_len", "stats"):
            assert np.array_equal(getattr(last, k).cpu().numpy(), getattr(want, k)), k
        res["restatement_agrees"] = True
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
