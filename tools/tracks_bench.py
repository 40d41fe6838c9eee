#!/usr/bin/env python
"""Times gtsfm_tracks_from_matches (2D feature tracks by union-find) on a synthetic C4-shaped input.

The input is built on the GPU from a seed: --images x --keypoints, every image pair, verified rows drawn from
--points latent 3D points (point j is seen by an image with probability vis * (1 - 0.95 u_j), so track lengths are
mixed; an image gives the points it sees consecutive keypoint slots) and a share --wrong-share of rows whose second
keypoint is replaced by a random one. A launch (workspace memset + union + flatten + two scans + place + rank +
scatter) is timed with HIP events around `inner` back-to-back launches, `inner` chosen after the warm-up so that a
timed window lasts at least --window-ms; the per-launch median, min and max over --repeats windows are reported. That
is a warm steady state: the 8 MB parent array lives in L2 / the Infinity Cache, the rows (larger than the cache at C4)
stream from HBM. Also reported: rows/s and the achieved fraction of the one-pass floor, the bytes of d_v_corr and
d_offsets divided by --hbm-tbps.
Two launches on the same input must give byte-identical outputs (asserted at the timed size), and with
--restatement the numpy / scipy restatement (tests/tracks_ref.py) runs on the same input: its time is reported, the
five counters must agree and --check-tracks random tracks are compared measurement by measurement.

    python tools/tracks_bench.py [--images 1000 --keypoints 2048] --restatement [--out bench_out/tracks.jsonl]
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

import tracks_ref as ref  # noqa: E402
from gtsfm_amd import device, native  # noqa: E402


def make_device_scene(n_img: int, kmax: int, n_points: int, vis: float, wrong_share: float, seed: int, dev):
    """(pairs (P, 2) int32, offsets (P + 1,) int32, v_corr (rows, 2) int32, kp_count, kp_xy) on the device."""
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    p_point = vis * (1.0 - 0.95 * torch.rand(n_points, device=dev, generator=gen))
    seen = torch.rand((n_img, n_points), device=dev, generator=gen) < p_point[None, :]
    slot = torch.cumsum(seen, dim=1, dtype=torch.int32) - 1
    seen &= slot < kmax
    chunks, counts = [], []
    for i in range(n_img - 1):
        common = seen[i][None, :] & seen[i + 1:]
        dj, pt = torch.nonzero(common, as_tuple=True)  # by second image, then point
        chunks.append(torch.stack([slot[i, pt], slot[i + 1 + dj, pt]], dim=1))
        counts.append(common.sum(dim=1))
    v_corr = torch.cat(chunks).to(torch.int32)
    del chunks
    wrong = torch.rand(v_corr.shape[0], device=dev, generator=gen) < wrong_share
    v_corr[wrong, 1] = torch.randint(0, kmax, (int(wrong.sum()),), device=dev, generator=gen, dtype=torch.int32)
    iu = torch.triu_indices(n_img, n_img, offset=1, device=dev)
    pairs = iu.t().contiguous().to(torch.int32)  # (i1, i2) ascending, i2 fastest: the order of `counts`
    offsets = torch.zeros(pairs.shape[0] + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(torch.cat(counts), dim=0)
    assert int(offsets[-1]) == v_corr.shape[0] < 2 ** 31
    kp_xy = torch.rand((n_img, kmax, 2), device=dev, generator=gen) * 1000.0
    kp_count = torch.full((n_img,), kmax, dtype=torch.int32, device=dev)  # a wrong row may name any slot
    return pairs, offsets.to(torch.int32), v_corr.contiguous(), kp_count, kp_xy


def time_launches(fn, warmup: int, repeats: int, window_ms: float):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    inner = max(1, int(np.ceil(window_ms / max(start.elapsed_time(stop), 1e-3))))
    per_launch = []
    for _ in range(repeats):
        start.record()
        for _ in range(inner):
            fn()
        stop.record()
        stop.synchronize()
        per_launch.append(start.elapsed_time(stop) / inner)
    return inner, per_launch


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--keypoints", type=int, default=2048)
    ap.add_argument("--points", type=int, default=60000)
    ap.add_argument("--vis", type=float, default=0.06)
    ap.add_argument("--wrong-share", type=float, default=0.002)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--hbm-tbps", type=float, default=8.0, help="HBM bandwidth the one-pass floor is taken at")
    ap.add_argument("--restatement", action="store_true", help="run and time tests/tracks_ref.py on the same input")
    ap.add_argument("--check-tracks", type=int, default=2000)
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
    pairs, offsets, v_corr, kp_count, kp_xy = make_device_scene(args.images, args.keypoints, args.points, args.vis,
                                                                args.wrong_share, args.seed, dev)
    torch.cuda.synchronize()
    rows, P = v_corr.shape[0], pairs.shape[0]
    print(f"scene: {args.images} images x {args.keypoints} keypoints, {P} pairs, {rows} rows "
          f"({time.perf_counter() - t0:.1f} s to build)", flush=True)
    need = native.lib().gtsfm_tracks_workspace_bytes(args.images, args.keypoints, P, rows)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = {}

    def launch(buffers=None):
        out["r"] = device.tracks_from_matches(pairs, offsets, v_corr, kp_count, args.keypoints, kp_xy=kp_xy,
                                              workspace=ws, out=buffers)

    launch()
    first = [a.clone() for a in out["r"]]
    inner, ms = time_launches(lambda: launch(out["r"][:4]), args.warmup, args.repeats, args.window_ms)
    stats = out["r"][4].cpu().numpy()
    n_tracks, n_meas = int(stats[0]), int(stats[1])
    # determinism at the timed size: a fresh launch into fresh buffers against the very first one
    launch()
    for a, b, n in zip(first, out["r"], (n_tracks + 1, n_meas, n_meas, n_meas, 5)):
        assert torch.equal(a[:n], b[:n]), "two launches on the same input differ"
    med = statistics.median(ms)
    floor_ms = (rows * 8 + (P + 1) * 4) / (args.hbm_tbps * 1e12) * 1e3
    lengths = torch.diff(out["r"][0][: n_tracks + 1])
    emit({"what": "gtsfm_tracks_from_matches", "images": args.images, "keypoints": args.keypoints, "pairs": P,
          "rows": rows, "wrong_share": args.wrong_share, "n_tracks": n_tracks, "n_measurements": n_meas,
          "n_components": int(stats[2]), "n_erroneous": int(stats[3]), "n_bad_rows": int(stats[4]),
          "longest_track": int(lengths.max()) if n_tracks else 0, "workspace_bytes": need,
          "launch_ms_median": round(med, 4), "launch_ms_min": round(min(ms), 4), "launch_ms_max": round(max(ms), 4),
          "launches_per_window": inner, "windows": len(ms), "rows_per_s": round(rows / (med * 1e-3), 1),
          "one_pass_floor_ms": round(floor_ms, 4), "fraction_of_floor": round(floor_ms / med, 4),
          "byte_identical_relaunch": True})

    failed = False
    if args.restatement:
        h = [a.cpu().numpy() for a in (pairs, offsets, v_corr, kp_count)]
        t0 = time.perf_counter()
        want = ref.reference_tracks(h[0], h[1], h[2], h[3], args.keypoints, None, None)
        sec = time.perf_counter() - t0
        got_off = out["r"][0][: n_tracks + 1].cpu().numpy()
        got_img, got_kp = out["r"][1][:n_meas].cpu().numpy(), out["r"][2][:n_meas].cpu().numpy()
        stats_equal = bool(np.array_equal(stats, want.stats))
        ids = np.sort(np.random.default_rng(args.seed).permutation(int(want.stats[0]))[: args.check_tracks])
        tracks_equal = stats_equal
        if stats_equal:
            for t in ids:
                lo, hi = want.offsets[t], want.offsets[t + 1]
                tracks_equal &= bool(got_off[t] == lo and got_off[t + 1] == hi
                                     and np.array_equal(got_img[lo:hi], want.image[lo:hi])
                                     and np.array_equal(got_kp[lo:hi], want.keypoint[lo:hi]))
        uv = out["r"][3][:n_meas]
        uv_equal = bool(torch.equal(uv, kp_xy[out["r"][1][:n_meas].long(), out["r"][2][:n_meas].long()]))
        emit({"what": "numpy / scipy restatement (tests/tracks_ref.py), same input", "rows": rows,
              "seconds": round(sec, 3), "speedup_over_restatement": round(sec / (med * 1e-3), 1),
              "stats_equal": stats_equal, "checked_tracks": len(ids), "checked_tracks_equal": tracks_equal,
              "uv_is_the_gather": uv_equal})
        failed = not (stats_equal and tracks_equal and uv_equal)

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    if failed:
        raise SystemExit("the kernel disagrees with the restatement")


if __name__ == "__main__":
    main()
