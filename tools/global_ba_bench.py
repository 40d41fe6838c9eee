#!/usr/bin/env python
"""Times gtsfm_global_ba (bundle adjustment of all cameras and landmarks) on a synthetic C4-shaped scene.

Scene: tests/global_ba_ref.ring_scene with --images cameras on a ring, --tracks landmarks each seen by 10-19 cameras
(about 14.5 measurements per track: 1000 cameras, 14,000 tracks and 205,000 measurements, the shape tools/tracks_bench.py
produces at C4), 0.5 px noise, 5 % of the measurements displaced by 30 px, perturbed cameras and landmarks. The call is
robust, --max-iterations LM iterations. It synchronises its stream, so a call is timed with a host clock around it
(after a warm-up call); reported: ms per call (median, min, max over --repeats), per LM trial and per PCG iteration,
PCG iterations per solve, and the product's algorithmic bytes. The PCG iteration (two product kernels, the vector
step, one 48-byte read-back) is timed by difference: two calls of one LM iteration whose solves are capped at --cap-a and
--cap-b products differ by exactly (cap-b - cap-a) iterations per trial. Bytes over that time is a lower bound on the
product kernels' rate, since the vector step and the read-back are inside it. Two calls must be byte-identical. With
--restatement the numpy restatement (tests/global_ba_ref.py) and the kernel both run a --sample-images camera scene of
the same generator and must agree.

--refine-calibration {per-camera,shared} also times gtsfm_global_ba_calib (calibration refined, prior sigma
--calibration-sigma) on the same input in the same run, f stored as (f, 0, 0, u0, v0), and reports its call time, its
time per PCG iteration and both as a ratio to the fixed-calibration call; with --restatement it is checked against
tests/global_ba_calib_ref.py on the sample scene seen by a distorted camera.

    python tools/global_ba_bench.py [--images 1000] --restatement [--out bench_out/global_ba.jsonl]
    python tools/global_ba_bench.py --refine-calibration per-camera --restatement
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
sys.path.insert(0, os.path.join(REPO, "tests"))

import global_ba_calib_ref as cref  # noqa: E402
import global_ba_ref as ref  # noqa: E402
from gtsfm_amd import device, native  # noqa: E402

# gba.hip per factor measurement and product: pass 1 reads Jx, Jp (144 B of the 160 B record), the camera's p (48 B), the
# image index (4 B); pass 2 reads Jx, Jp (144 B), the track's y (24 B), the camera-major index and the track index (8 B)
PRODUCT_BYTES_PER_MEASUREMENT = 144 + 48 + 4 + 144 + 24 + 8
FIELDS = ("wRc", "wtc", "point", "track_keep", "cam_keep", "stats")  # of a result, compared byte for byte


def to_dev(s, dev):
    def t(a, dtype=None):
        return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))).to(dev)

    return (t(s["offsets"], np.int32), t(s["img"], np.int32), t(s["uv"].astype(np.float32)), t(s["point"]),
            t(s["track_valid"], np.uint8), t(s["meas_valid"], np.uint8), t(s["wRc"]), t(s["wtc"]), t(s["intr"]),
            t(s["cam_valid"], np.uint8))


def timed(args, fn, **kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn(*args, **kw)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def time_solver(a, fn, args, fields, **kw):
    """What both solvers are measured by: a warm-up call, --repeats timed calls, the byte-identity of `fields` between
    the warm-up and the last call, and the PCG iteration by difference (one LM iteration whose solves are capped at
    --cap-a and --cap-b; both caps must bind for the difference to be exact). Returns the call times, the last call's
    stats and the ms per PCG iteration (nan when no pair of calls was comparable)."""
    _, warm = timed(args, fn, max_iterations=a.max_iterations, **kw)
    times, last = [], None
    for _ in range(a.repeats):
        ms, last = timed(args, fn, max_iterations=a.max_iterations, **kw)
        times.append(ms)
    for k in fields:
        assert getattr(warm, k).cpu().numpy().tobytes() == getattr(last, k).cpu().numpy().tobytes(), k
    diff = []
    for _ in range(a.repeats):
        ta, ra = timed(args, fn, max_iterations=1, pcg_max_iter=a.cap_a, **kw)
        tb, rb = timed(args, fn, max_iterations=1, pcg_max_iter=a.cap_b, **kw)
        sa, sb = ra.stats.cpu().numpy(), rb.stats.cpu().numpy()
        if sa[3] == sb[3] and sb[4] > sa[4]:
            diff.append((tb - ta) / (sb[4] - sa[4]))
    return times, last.stats.cpu().numpy(), statistics.median(diff) if diff else float("nan")


def refine_calibration_bench(a, s, args, dev, fixed):
    """gtsfm_global_ba_calib on the input the fixed-calibration call was just timed on: call time, time per PCG
    iteration by the same difference of two caps, both against `fixed`; with --restatement the sample-scene check."""
    shared = a.refine_calibration == "shared"
    K = s["intr"]
    calib = torch.from_numpy(np.concatenate([K[:, :1], np.zeros((len(K), 2)), K[:, 1:]], 1)).to(dev)
    cargs = args[:8] + (calib,) + args[9:]
    n_meas = len(s["img"])
    ws = torch.empty(native.lib().gtsfm_global_ba_calib_workspace_bytes(a.tracks, n_meas, a.images),
                     dtype=torch.uint8, device=dev)
    times, st, per_iter = time_solver(a, device.global_ba_calib, cargs, FIELDS + ("calib",), robust=True,
                                      reproj_error_thresh=3.0, workspace=ws, shared_calib=shared,
                                      calibration_prior_sigma=a.calibration_sigma)
    out = {"refine_calibration": a.refine_calibration, "calibration_sigma": a.calibration_sigma,
           "calib_call_ms_median": statistics.median(times), "calib_call_ms_min": min(times),
           "calib_lm_iterations": st[2], "calib_lm_trials": st[3], "calib_pcg_iterations": st[4],
           "calib_ms_per_lm_trial": statistics.median(times) / max(st[3], 1), "calib_ms_per_pcg_iteration": per_iter,
           "calib_final_error": st[1], "calib_variables": st[10], "calib_max_rel_focal_change": st[11],
           "calib_byte_identical": True,
           "calib_over_fixed_call": statistics.median(times) / fixed["call_ms_median"],
           "calib_over_fixed_lm_trial": (statistics.median(times) / max(st[3], 1)) / fixed["ms_per_lm_trial"],
           "calib_over_fixed_pcg_iteration": per_iter / fixed["ms_per_pcg_iteration"]}
    if a.restatement:
        s2 = cref.distort_scene(ref.ring_scene(a.sample_images, 15 * a.sample_images, 4, 9, a.seed + 1))
        s2["uv"] = s2["uv"].astype(np.float32).astype(np.float64)
        opts = dict(robust=True, max_iterations=a.max_iterations, reproj_error_thresh=3.0, shared_calib=shared,
                    calibration_prior_sigma=a.calibration_sigma)
        want = cref.global_ba_calib_ref(*cref.call_args(s2), **opts)
        d2 = to_dev(s2, dev)
        got = device.global_ba_calib(*d2[:8], torch.from_numpy(s2["calib"]).to(dev), *d2[9:], **opts)
        gs = got.stats.cpu().numpy()
        cams = np.arange(a.sample_images)
        rot, tr = ref.pose_diff(got.wRc.cpu().numpy(), got.wtc.cpu().numpy(), want.wRc, want.wtc, cams)
        df, dk = cref.calib_diff(got.calib.cpu().numpy(), want.calib, cams)
        out.update(calib_sample_rot_deg=rot, calib_sample_trans_rel=tr, calib_sample_f_rel=df, calib_sample_k_abs=dk,
                   calib_sample_lm_counts_equal=bool((gs[2:4] == want.stats[2:4]).all()),
                   calib_sample_keep_equal=bool(np.array_equal(got.track_keep.cpu().numpy(), want.track_keep)),
                   calib_sample_ref_margin=want.min_margin)
        assert rot <= 1e-4 and tr <= 1e-6 and df <= 1e-6 and dk <= 1e-6, (rot, tr, df, dk)
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--tracks", type=int, default=14000)
    ap.add_argument("--max-iterations", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cap-a", type=int, default=20)
    ap.add_argument("--cap-b", type=int, default=120)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--restatement", action="store_true")
    ap.add_argument("--sample-images", type=int, default=40)
    ap.add_argument("--refine-calibration", choices=("off", "per-camera", "shared"), default="off")
    ap.add_argument("--calibration-sigma", type=float, default=50.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    native.require_gpu()
    dev = torch.device("cuda:0")
    s = ref.ring_scene(a.images, a.tracks, 10, 19, a.seed)
    args = to_dev(s, dev)
    n_meas = len(s["img"])
    ws = torch.empty(native.lib().gtsfm_global_ba_workspace_bytes(a.tracks, n_meas, a.images), dtype=torch.uint8,
                     device=dev)
    times, st, per_iter_ms = time_solver(a, device.global_ba, args, FIELDS, robust=True, reproj_error_thresh=3.0,
                                         workspace=ws)
    factors = n_meas  # every measurement is a factor in this scene
    product_bytes = PRODUCT_BYTES_PER_MEASUREMENT * factors
    res = {
        "tool": "global_ba_bench", "images": a.images, "tracks": a.tracks, "measurements": n_meas,
        "max_iterations": a.max_iterations, "call_ms_median": statistics.median(times), "call_ms_min": min(times),
        "call_ms_max": max(times), "lm_iterations": st[2], "lm_trials": st[3], "pcg_iterations": st[4],
        "pcg_cap_hits": st[5], "pcg_iterations_per_solve": st[4] / max(st[3], 1),
        "ms_per_lm_trial": statistics.median(times) / max(st[3], 1), "ms_per_pcg_iteration": per_iter_ms,
        "product_algorithmic_bytes": product_bytes,
        "product_bytes_per_s_lower_bound": None if np.isnan(per_iter_ms) else product_bytes / (per_iter_ms * 1e-3),
        "initial_error": st[0], "final_error": st[1], "tracks_kept": st[8], "byte_identical": True,
    }
    if a.refine_calibration != "off":
        res.update(refine_calibration_bench(a, s, args, dev, res))
    if a.restatement:
        s2 = ref.ring_scene(a.sample_images, 15 * a.sample_images, 4, 9, a.seed + 1)
        t0 = time.perf_counter()
        want = ref.global_ba_ref(*ref.call_args(dict(s2, uv=s2["uv"].astype(np.float32).astype(np.float64))),
                                 robust=True, max_iterations=a.max_iterations, reproj_error_thresh=3.0)
        res["restatement_s"] = time.perf_counter() - t0
        got = device.global_ba(*to_dev(s2, dev), robust=True, max_iterations=a.max_iterations, reproj_error_thresh=3.0)
        gs = got.stats.cpu().numpy()
        rot, tr = ref.pose_diff(got.wRc.cpu().numpy(), got.wtc.cpu().numpy(), want.wRc, want.wtc,
                                np.arange(a.sample_images))
        res.update(sample_images=a.sample_images, sample_rot_deg=rot, sample_trans_rel=tr,
                   sample_lm_counts_equal=bool((gs[2:4] == want.stats[2:4]).all()),
                   sample_keep_equal=bool(np.array_equal(got.track_keep.cpu().numpy(), want.track_keep)),
                   sample_ref_margin=want.min_margin)
        assert rot <= 1e-4 and tr <= 1e-6, (rot, tr)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
