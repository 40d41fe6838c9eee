#!/usr/bin/env python
"""Times gtsfm_triangulate_tracks (tracks to 3D landmarks) on a synthetic C4-shaped scene.

Scene: --images cameras on a ring looking at a ball of points; 2D tracks come from the correspondences of
tests/tracks_ref.make_scene (visibility spread, so track lengths are mixed) through gtsfm_tracks_from_matches, and
every measurement is the projection of its track's latent point plus --noise px, a share --outlier-share of them moved
by 50-150 px. The launch uses the shipped options (RANSAC_SAMPLE_UNIFORM, max_num_hypotheses 100, threshold 3 px).
A launch (scan + select + score + finish, every chunk) is timed with HIP events around `inner` back-to-back launches,
`inner` chosen after the warm-up so that a timed window lasts at least --window-ms; the per-launch median, min and max
over --repeats windows, hypotheses per second and the exit-code histogram are reported. Two launches must be
byte-identical. With --restatement the numpy restatement (tests/triangulation_ref.py) runs on --sample tracks: its time
is reported and its exit codes must agree outside the near-ties.

    python tools/triangulate_bench.py [--images 1000] --restatement [--out bench_out/triangulate.jsonl]
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

import tracks_ref  # noqa: E402
import triangulation_ref as ref  # noqa: E402
from gtsfm_amd import device, native  # noqa: E402
from tracks_bench import time_launches  # noqa: E402


def make_scene(n_img, kp_per_img, n_points, vis, noise, outlier_share, seed):
    """(offsets, image, uv float32, cams): tracks of tests/tracks_ref.make_scene's correspondences, grouped by the
    restatement of the tracks kernel, with measurements of seeded latent points."""
    rng = np.random.default_rng(seed)
    scene = tracks_ref.make_scene(n_img, kp_per_img, n_points, vis, seed=seed, vis_spread=0.95)
    tr = tracks_ref.reference_tracks(scene.pairs, scene.offsets, scene.v_corr, scene.kp_count, scene.kmax)
    th = np.linspace(0, 2 * np.pi, n_img, endpoint=False)
    cams = ref.lookat_cameras(np.stack([10 * np.cos(th), 10 * np.sin(th), rng.uniform(-1.5, 1.5, n_img)], axis=1))
    T = len(tr.offsets) - 1
    X = rng.normal(size=(T, 3))
    X = X / np.linalg.norm(X, axis=1, keepdims=True) * rng.uniform(0, 2, (T, 1))
    track_of = np.repeat(np.arange(T), np.diff(tr.offsets))
    uv, _ = ref.project(cams, tr.image, X[track_of])
    bad = rng.random(len(uv)) < outlier_share
    ang = rng.uniform(0, 2 * np.pi, len(uv))
    shift = rng.uniform(50, 150, len(uv))[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    uv = uv + np.where(bad[:, None], shift, rng.normal(scale=noise, size=uv.shape))
    return tr.offsets, tr.image, uv.astype(np.float32), cams


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--keypoints", type=int, default=256)
    ap.add_argument("--points", type=int, default=14000)
    ap.add_argument("--vis", type=float, default=0.012)
    ap.add_argument("--noise", type=float, default=0.5)
    ap.add_argument("--outlier-share", type=float, default=0.1)
    ap.add_argument("--n-hyp", type=int, default=100)
    ap.add_argument("--threshold", type=float, default=3.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--restatement", action="store_true", help="run and time tests/triangulation_ref.py on a subsample")
    ap.add_argument("--sample", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    args = ap.parse_args()
    native.require_gpu()
    dev = torch.device("cuda:0")
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    t0 = time.perf_counter()
    off, img, uv, cams = make_scene(args.images, args.keypoints, args.points, args.vis, args.noise,
                                    args.outlier_share, args.seed)
    T, n_meas = len(off) - 1, len(img)
    print(f"scene: {args.images} cameras, {T} tracks, {n_meas} measurements, longest {int(np.diff(off).max())} "
          f"({time.perf_counter() - t0:.1f} s to build)", flush=True)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d = [t(off.astype(np.int32)), t(img.astype(np.int32)), t(uv), t(cams.wRc), t(cams.wtc), t(cams.intr)]
    need = native.lib().gtsfm_triangulate_workspace_bytes(T, n_meas, args.n_hyp)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = {}

    def launch():
        out["r"] = device.triangulate_tracks(*d, None, native.GTSFM_TRI_RANSAC_SAMPLE_UNIFORM, args.threshold, 0.0,
                                             args.n_hyp, args.seed, workspace=ws)

    launch()
    first = out["r"]
    inner, ms = time_launches(launch, args.warmup, args.repeats, args.window_ms)
    for k in ("exit_code", "point", "avg_err", "inlier", "stats"):
        a, b = getattr(first, k).cpu().numpy(), getattr(out["r"], k).cpu().numpy()
        assert a.tobytes() == b.tobytes(), f"two launches differ in {k}"
    stats = out["r"].stats.cpu().numpy()
    med = statistics.median(ms)
    emit({"what": "gtsfm_triangulate_tracks", "images": args.images, "tracks": T, "measurements": n_meas,
          "n_hyp": args.n_hyp, "threshold": args.threshold, "hypotheses": int(stats[7]), "workspace_bytes": need,
          "exit_codes": dict(zip(native.TRI_STATS_FIELDS[:6], stats[:6].tolist())),
          "inlier_measurements": int(stats[6]), "launch_ms_median": round(med, 4), "launch_ms_min": round(min(ms), 4),
          "launch_ms_max": round(max(ms), 4), "launches_per_window": inner, "windows": len(ms),
          "hypotheses_per_s": round(int(stats[7]) / (med * 1e-3), 1), "byte_identical_relaunch": True})
    failed = False
    if args.restatement:
        n = min(args.sample, T)
        m = int(off[n])
        t0 = time.perf_counter()
        want = ref.triangulate_tracks(off[: n + 1], img[:m], uv[:m], cams, ref.UNIFORM, args.threshold,
                                      n_hyp=args.n_hyp, seed=args.seed)
        sec = time.perf_counter() - t0
        keep = ~want.margins.near_tie(1e-6)
        got = out["r"].exit_code.cpu().numpy()[:n]
        equal = bool(np.array_equal(got[keep], want.exit_code[keep]))
        emit({"what": "numpy restatement (tests/triangulation_ref.py), first tracks of the same input", "tracks": n,
              "seconds": round(sec, 3), "near_ties": int((~keep).sum()), "exit_codes_equal": equal,
              "restatement_s_per_track": round(sec / max(n, 1), 6), "kernel_s_per_track": round(med * 1e-3 / T, 9)})
        failed = not equal
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    if failed:
        raise SystemExit("the kernel disagrees with the restatement")


if __name__ == "__main__":
    main()
