#!/usr/bin/env python
"""Times the three gtsfm_transavg_* stages (1DSfM translation averaging) on a synthetic scene.

Scene: tests/translation_averaging_ref.seeded_scene with --images cameras on a perturbed ring, each pair an edge with
probability --edge-frac (noisy directions, --outlier-frac of them replaced by random ones) and --points landmarks seen
by 2-6 cameras each, from which the selection keeps about 12 track measurements per camera. Reported: milliseconds per
launch of the measurements, MFAS (--directions projection directions) and recovery stages (median, min and max over
--repeats windows, each one launch bracketed by device synchronisation, after a warm-up), and MFAS directions per
second. Two launches of every stage must be byte-identical. With --restatement the sequential numpy MFAS
(tests/translation_averaging_ref.py) runs --sample-directions of the directions on the same graph; their violated sets
must equal the kernel's, and its time is reported.

    python tools/translation_averaging_bench.py [--images 1000] --restatement [--out bench_out/translation_averaging.jsonl]
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

import translation_averaging_ref as ref  # noqa: E402
from gtsfm_amd import device, native  # noqa: E402


def windows(fn, repeats):
    fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out)}, r


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--edge-frac", type=float, default=0.03)
    ap.add_argument("--outlier-frac", type=float, default=0.1)
    ap.add_argument("--directions", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--restatement", action="store_true")
    ap.add_argument("--sample-directions", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    native.require_gpu()
    dev = torch.device("cuda:0")
    s = ref.seeded_scene(a.images, a.seed, n_pts=a.points, edge_frac=a.edge_frac, outlier_frac=a.outlier_frac)

    def t(x):
        return torch.from_numpy(np.ascontiguousarray(x)).to(dev)

    args = (t(s["edges"]), t(s["i2Ui1"]), None, t(s["wRi"]), None, t(s["offsets"]), t(s["img"]), t(s["uv"]), t(s["intr"]))
    res = {"images": a.images, "edges": len(s["edges"]), "tracks": a.points, "directions": a.directions}
    res["measurements"], ms = windows(lambda: device.transavg_measurements(*args), a.repeats)
    ms2 = device.transavg_measurements(*args)
    same = all(torch.equal(getattr(ms, f), getattr(ms2, f)) for f in ("key", "dir", "valid", "selected", "counts"))
    counts = ms.counts.cpu().numpy()
    n, n_land = len(s["edges"]) + int(counts[1]), int(counts[2])
    n_nodes = a.images + n_land
    res.update(measurements_in_use=n, selected_tracks=n_land, nodes=n_nodes)
    key, d, valid = ms.key[:n].contiguous(), ms.dir[:n].contiguous(), ms.valid[:n].contiguous()
    proj = t(ref.sample_uniform_directions(a.directions, a.seed))
    res["mfas"], mf = windows(lambda: device.transavg_mfas(key, d, valid, n_nodes, proj, want_violated=True), a.repeats)
    mf2 = device.transavg_mfas(key, d, valid, n_nodes, proj, want_violated=True)
    same = same and all(torch.equal(x, y) for x, y in zip(mf, mf2))
    res["mfas"]["directions_per_s"] = a.directions / (res["mfas"]["median_ms"] * 1e-3)
    res["inlier_camera_edges"] = int(mf[1][: len(s["edges"])].sum().item())
    res["planted_outlier_edges"] = int(s["outlier"].sum())
    res["recover"], rec = windows(lambda: device.transavg_recover(key, d, mf[1], a.images, n_land, seed=a.seed),
                                  max(a.repeats // 2, 1))
    rec2 = device.transavg_recover(key, d, mf[1], a.images, n_land, seed=a.seed)
    same = same and torch.equal(rec.wti.view(torch.uint8), rec2.wti.view(torch.uint8)) and \
        torch.equal(rec.stats.view(torch.uint8), rec2.stats.view(torch.uint8))
    res["recover"]["stats"] = dict(zip(native.TA_STATS_FIELDS, rec.stats.cpu().numpy().tolist()))
    res["byte_identical"] = bool(same)
    aligned = ref.align_sim3(s["wti"], rec.wti.cpu().numpy())
    res["max_position_error_after_alignment"] = float(np.abs(aligned - s["wti"]).max())
    if a.restatement:
        only = list(range(0, a.directions, max(a.directions // a.sample_directions, 1)))[: a.sample_directions]
        t0 = time.perf_counter()
        want = ref.mfas(key.cpu().numpy(), d.cpu().numpy(), valid.cpu().numpy(), n_nodes, proj.cpu().numpy(), only=only)
        dt = time.perf_counter() - t0
        mask = ref.violated_bits_to_mask(mf[2].cpu().numpy().view(np.uint32)[only], n)
        near = want.margins < ref.NEAR_TIE
        ok = all(np.array_equal(mask[i], want.violated[i]) for i in range(len(only)) if not near[i])
        res["restatement"] = {"directions": only, "seconds": dt, "seconds_per_direction": dt / len(only),
                              "near_ties": int(near.sum()), "violated_sets_equal": bool(ok)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    if not same or (a.restatement and not res["restatement"]["violated_sets_equal"]):
        sys.exit(1)


if __name__ == "__main__":
    main()
