#!/usr/bin/env python
"""The float-descriptor matcher timed on the MI355X: GTSFM_MATCH_F16_RERANK (fp16 MFMA shortlist + certified exact
re-rank) against GTSFM_MATCH_EXACT_F32 on the same planted unit descriptors, in one process, with HIP events after a
warm-up of both modes and the two modes alternating. Both modes give the same matches (checked on every pair), so the
ratio is the price of not having the shortlist at this width. Prints one JSON line: ms per pair (median and the
min .. max spread over the repeats), the ratio, the same with the spreads against it (`ratio_worst`), and the
certificate's statistics. --restatement also checks the first pairs against a float64 numpy restatement of mutual
nearest neighbours + ratio test.

    python tools/match_float_bench.py --dim 512 --kpts 5000 --images 8 --restatement
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from gtsfm_amd import device, native  # noqa: E402


def planted_views(rng, n_images, kpts, dim, frac=0.3, noise=0.15):
    """Random unit descriptors; a share `frac` of every view are noisy copies of rows of one latent set, so every
    pair of views has planted matches."""
    def unit(n):
        x = rng.normal(size=(n, dim))
        return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)

    base = unit(kpts)
    k = int(frac * kpts)
    views = []
    for _ in range(n_images):
        d = unit(kpts)
        y = base[rng.permutation(kpts)[:k]] + noise * rng.normal(size=(k, dim)) / np.sqrt(dim)
        d[rng.permutation(kpts)[:k]] = y / np.linalg.norm(y, axis=1, keepdims=True)
        views.append(d)
    return np.stack(views)


def restatement(a, b, ratio):
    """Mutual nearest neighbours + ratio test in float64: (matches (M, 2) by ascending distance, their distances)."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    d2 = np.maximum((a ** 2).sum(1)[:, None] + (b ** 2).sum(1)[None, :] - 2.0 * a @ b.T, 0.0)

    def oneway(m):
        j1 = m.argmin(1)
        two = np.sqrt(np.partition(m, 1, axis=1)[:, :2]) if m.shape[1] > 1 else None
        ok = np.ones(len(m), bool) if ratio is None or two is None else two[:, 0] <= ratio * two[:, 1]
        return j1, ok

    j12, ok12 = oneway(d2)
    j21, ok21 = oneway(d2.T)
    i = np.nonzero(ok12 & (j21[j12] == np.arange(len(a))) & ok21[j12])[0]
    dist = np.sqrt(d2[i, j12[i]])
    order = np.argsort(dist, kind="stable")
    return np.stack([i[order], j12[i[order]]], 1), dist[order]


def check_restatement(got, a, b, ratio):
    """Same set of matches, and the device's order ascending in the restatement's distances (to float32 rounding:
    the device sorts float32 distances, so two matches whose distances round together may swap)."""
    ref, _ = restatement(a, b, ratio)
    got = got.reshape(-1, 2).astype(np.int64)
    same_set = np.array_equal(got[np.lexsort((got[:, 1], got[:, 0]))], ref[np.lexsort((ref[:, 1], ref[:, 0]))])
    d = np.linalg.norm(a[got[:, 0]].astype(np.float64) - b[got[:, 1]].astype(np.float64), axis=1)
    return bool(same_set and (np.diff(d) > -1e-6).all())


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--kpts", type=int, default=5000)
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--ratio", type=float, default=0.8)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--restatement", action="store_true")
    args = ap.parse_args()
    native.require_gpu()
    dev = torch.device("cuda:0")
    n, k, dim = args.images, args.kpts, args.dim
    host = planted_views(np.random.default_rng(args.seed), n, k, dim)
    desc = torch.from_numpy(host).to(dev)
    counts = torch.full((n,), k, dtype=torch.int32, device=dev)
    pair_list = [(i, j) for i in range(n) for j in range(i + 1, n)]
    pairs = torch.tensor(pair_list, dtype=torch.int32, device=dev)
    P = len(pair_list)
    modes = {"f16_rerank": native.GTSFM_MATCH_F16_RERANK, "exact_f32": native.GTSFM_MATCH_EXACT_F32}
    outs = {m: (torch.empty((P, k, 2), dtype=torch.int32, device=dev),
                torch.zeros((P,), dtype=torch.int32, device=dev)) for m in modes}
    stats = {}
    for m, mode in modes.items():  # warm-up of both: code objects, first launches, workspaces
        device.match_pairs(desc, counts, pairs, args.ratio, mode, out=outs[m], stats=stats)
    torch.cuda.synchronize()
    cnt = {m: outs[m][1].cpu().numpy() for m in modes}
    idx = {m: outs[m][0].cpu().numpy() for m in modes}
    identical = bool(np.array_equal(cnt["f16_rerank"], cnt["exact_f32"]) and all(
        np.array_equal(idx["f16_rerank"][p, : cnt["exact_f32"][p]], idx["exact_f32"][p, : cnt["exact_f32"][p]])
        for p in range(P)))
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = {m: [] for m in modes}
    for _ in range(args.repeats):  # alternating, so a busy spell on the host or the device hits both
        for m, mode in modes.items():
            start.record()
            device.match_pairs(desc, counts, pairs, args.ratio, mode, out=outs[m])
            stop.record()
            torch.cuda.synchronize()
            ms[m].append(start.elapsed_time(stop) / P)
    line = {"tool": "match_float_bench", "dim": dim, "kpts": k, "images": n, "pairs": P, "ratio": args.ratio,
            "repeats": args.repeats, "matches_identical": identical,
            "matches_per_pair": round(float(cnt["exact_f32"].mean()), 1)}
    for m in modes:
        line[m + "_ms_per_pair"] = round(float(np.median(ms[m])), 4)
        line[m + "_ms_spread"] = [round(float(min(ms[m])), 4), round(float(max(ms[m])), 4)]
    line["ratio_exact_over_f16"] = round(float(np.median(ms["exact_f32"]) / np.median(ms["f16_rerank"])), 2)
    line["ratio_worst"] = round(float(min(ms["exact_f32"]) / max(ms["f16_rerank"])), 2)  # spreads against the claim
    line["certificate"] = {key: (round(v, 6) if isinstance(v, float) else v) for key, v in stats.items()}
    ok = identical
    if args.restatement:
        n_check = min(2, P)
        good = [check_restatement(idx["f16_rerank"][p, : cnt["f16_rerank"][p]].view(np.uint32),
                                  host[pair_list[p][0]], host[pair_list[p][1]], args.ratio) for p in range(n_check)]
        line["restatement_pairs"] = n_check
        line["restatement_ok"] = bool(all(good))
        ok = ok and all(good)
    print(json.dumps(line))
    if not ok:
        raise SystemExit("matches differ between the modes or from the restatement")


if __name__ == "__main__":
    main()
