#!/usr/bin/env python
"""Times gtsfm_viewgraph_cycle_filter (the cycle-consistent rotation view-graph filter) on complete graphs.

For every --images size: a seeded complete graph of noisy relative rotations with a share of gross outliers
(tests/viewgraph_ref.py:make_scene), both aggregation criteria. A launch (workspace memset + lookup fill + one
workgroup per edge + triplet total) is timed with HIP events around `inner` back-to-back launches, `inner` chosen
after the warm-up so that a timed window lasts at least --window-ms; the per-launch median, min and max over
--repeats windows are reported, one JSON line per (size, criterion). That is a warm steady-state time: the rotation
table stays in the Infinity Cache from launch to launch. cold_launch_ms_* times single launches, each after a 512 MiB
fill has evicted the inputs, as a pipeline that runs the filter once would see it. The last timed launch's results
for --check-edges random edges are compared with the restatement at the timed size (aggregates within 1e-9 degrees,
counts and keep exactly; a mismatch fails the run). --restatement N also times the numpy / scipy restatement on a
whole N-image complete graph and checks the kernel against it there.

    python tools/viewgraph_bench.py --images 100 1000 --restatement 300 [--out bench_out/viewgraph.jsonl]
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

import viewgraph_ref as ref  # noqa: E402
from gtsfm_amd import device, native  # noqa: E402

CRITERIA = {"MIN_EDGE_ERROR": native.GTSFM_VG_MIN_EDGE_ERROR, "MEDIAN_EDGE_ERROR": native.GTSFM_VG_MEDIAN_EDGE_ERROR}


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


def time_cold_launches(fn, flush: torch.Tensor, repeats: int):
    """One launch per window, after a fill of `flush` (larger than the 256 MiB Infinity Cache) has evicted the inputs:
    the launch as a pipeline sees it, once after the front-end."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for i in range(repeats):
        flush.fill_(i)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        out.append(start.elapsed_time(stop))
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, nargs="+", default=[100, 1000])
    ap.add_argument("--outlier-share", type=float, default=0.1)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--restatement", type=int, default=0, help="also time the numpy restatement at this many images")
    ap.add_argument("--check-edges", type=int, default=2000,
                    help="edges of every timed graph whose results are compared with the restatement (0 = none)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    args = ap.parse_args()
    native.require_gpu()
    dev = torch.device("cuda:0")
    lines = []
    failed = False
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for n_img in args.images:
        pairs, R = ref.make_scene(n_img, seed=args.seed, outlier_share=args.outlier_share)
        pairs_d, R_d = torch.from_numpy(pairs).to(dev), torch.from_numpy(R).to(dev)
        need = native.lib().gtsfm_viewgraph_workspace_bytes(n_img, len(pairs))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        for name, code in CRITERIA.items():
            out = {}

            def launch():
                out["r"] = device.viewgraph_cycle_filter(pairs_d, R_d, None, n_img, code, ref.ERROR_THRESHOLD,
                                                         workspace=ws)

            inner, ms = time_launches(launch, args.warmup, args.repeats, args.window_ms)
            cold = time_cold_launches(launch, flush, args.repeats)
            keep, agg, n_trip, total = out["r"]
            evals = int(n_trip.sum().item())
            med = statistics.median(ms)
            check = {}
            if args.check_edges:  # the timed launch's own output, at the timed size, against the restatement
                ids = np.sort(np.random.default_rng(args.seed).permutation(len(pairs))[: args.check_edges])
                want = ref.reference_filter_edges(pairs, R, ids, name)
                diff = np.abs(agg.cpu().numpy()[ids] - want.agg_error_deg)
                check = {"checked_edges": len(ids), "checked_max_abs_diff_deg": float(np.nanmax(diff)),
                         "checked_n_triplets_equal": bool(np.array_equal(n_trip.cpu().numpy()[ids], want.n_triplets)),
                         "checked_keep_equal": bool(np.array_equal(keep.cpu().numpy()[ids] != 0, want.keep)),
                         "checked_threshold_margin_deg": ref.threshold_margin(want)}
                failed = failed or not (check["checked_max_abs_diff_deg"] <= 1e-9 and check["checked_keep_equal"]
                                        and check["checked_n_triplets_equal"])
            emit({"what": "gtsfm_viewgraph_cycle_filter", "images": n_img, "edges": len(pairs), "criterion": name,
                  **check,
                  "triplets": int(total.item()), "cycle_evaluations": evals, "kept": int(keep.sum().item()),
                  "workspace_bytes": need, "launch_ms_median": round(med, 4), "launch_ms_min": round(min(ms), 4),
                  "launch_ms_max": round(max(ms), 4), "launches_per_window": inner, "windows": len(ms),
                  "cold_launch_ms_median": round(statistics.median(cold), 4), "cold_launch_ms_min": round(min(cold), 4),
                  "cold_launch_ms_max": round(max(cold), 4),
                  "evaluations_per_s": round(evals / (med * 1e-3), 1),
                  "gathered_bytes_per_s": round(evals * 2 * 72 / (med * 1e-3), 1)})

    if args.restatement:
        n_img = args.restatement
        pairs, R = ref.make_scene(n_img, seed=args.seed, outlier_share=args.outlier_share)
        t0 = time.perf_counter()
        cycles = ref.RefCycles(pairs, R)
        want = {name: cycles.filter(name) for name in CRITERIA}
        sec = time.perf_counter() - t0
        rec = {"what": "numpy restatement (tests/viewgraph_ref.py), both criteria", "images": n_img,
               "edges": len(pairs), "triplets": cycles.total_triplets, "seconds": round(sec, 3)}
        for name, code in CRITERIA.items():
            keep, agg, n_trip, total = device.viewgraph_cycle_filter(
                torch.from_numpy(pairs).to(dev), torch.from_numpy(R).to(dev), None, n_img, code, ref.ERROR_THRESHOLD)
            diff = np.abs(agg.cpu().numpy() - want[name].agg_error_deg)
            rec[f"max_abs_diff_deg_{name}"] = float(np.nanmax(diff))
            rec[f"keep_equal_{name}"] = bool(np.array_equal(keep.cpu().numpy().astype(bool), want[name].keep))
        emit(rec)

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    if failed:
        raise SystemExit("the kernel disagrees with the restatement on the checked edges")


if __name__ == "__main__":
    main()
