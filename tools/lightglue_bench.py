#!/usr/bin/env python
"""LightGlue matching (gtsfm_lightglue_batched) timed on the MI355X with HIP events after warm-up: all pairs of
--images images of --kpts SuperPoint-like keypoints (unit 256-D descriptors, a third of every image's points shared
with a common pool), seeded random weights (tests/lightglue_weights.py). Reported per pair, as the median of
--windows calls with min and max: full depth (depth_confidence = -1), adaptive depth with the planted exit layers
(and their distribution), and gtsfm_superglue_batched on the same inputs. --restatement also times
tests/lightglue_ref.py under torch-ROCm in fp32 on the same GPU over the first --restatement-pairs pairs.
The call has no stage hook, so no per-stage split is reported.

    python tools/lightglue_bench.py --images 32 --kpts 2048 --restatement
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from gtsfm_amd import device, native  # noqa: E402
from gtsfm_amd.frontend.matcher.lightglue_matcher import pack_lightglue_weights  # noqa: E402
from gtsfm_amd.frontend.matcher.superglue_matcher import pack_superglue_weights  # noqa: E402


def windows(fn, n):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(n):
        start.record()
        fn()
        stop.record()
        torch.cuda.synchronize()
        out.append(start.elapsed_time(stop))
    return out


def per_pair(ms, n_pairs):
    return {"median": round(float(np.median(ms)) / n_pairs, 4), "min": round(min(ms) / n_pairs, 4),
            "max": round(max(ms) / n_pairs, 4)}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--kpts", type=int, default=2048)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--restatement", action="store_true")
    ap.add_argument("--restatement-pairs", type=int, default=16)
    args = ap.parse_args()
    native.require_gpu()
    import lightglue_ref
    import lightglue_weights as lgw
    from superglue_cases import make_images, pack
    from superpoint_weights import superglue_state_dict

    n, k = args.images, args.kpts
    kmax = (k + 63) // 64 * 64
    dev = torch.device("cuda:0")
    hws = [(480, 640), (600, 800), (720, 540)]
    images = make_images([k] * n, [hws[i % 3] for i in range(n)], args.seed)
    # planted exit layers: every descriptor's component along the token heads' direction, per image
    alphas = [(lgw.ALPHA_EARLY, lgw.ALPHA_EARLY, lgw.ALPHA_MID, lgw.ALPHA_NEVER)[i % 4] for i in range(n)]
    g = lgw.direction()
    planted = []
    for s, a in zip(images, alphas):
        d = s.desc - np.outer(s.desc @ g, g)
        d = d / np.linalg.norm(d, axis=1, keepdims=True) * np.sqrt(1 - a * a) + a * g
        planted.append(s._replace(desc=d.astype(np.float32)))
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
    P = len(pairs)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    kp, sc, de, cnt, hw = (t(a) for a in pack(planted, kmax))
    pr = t(np.asarray(pairs, np.int32))
    sd = lgw.lightglue_state_dict(0)
    blob = t(pack_lightglue_weights(sd))
    L = native.lib()
    ws = torch.empty(L.gtsfm_lightglue_workspace_bytes(P, kmax), dtype=torch.uint8, device=dev)
    line = {"tool": "lightglue_bench", "images": n, "kpts": k, "pairs": P, "windows": args.windows,
            "workspace_MiB": round(ws.numel() / 2 ** 20, 1)}
    for name, conf in (("full_depth", -1.0), ("adaptive", 0.95)):
        run = lambda: device.lightglue_match(kp, de, cnt, hw, pr, blob, 9, conf, 0.1, workspace=ws)  # noqa: E731
        idx, c, _, ex = run()  # warm-up: code objects, first launches
        torch.cuda.synchronize()
        line[f"{name}_ms_per_pair"] = per_pair(windows(run, args.windows), P)
        line[f"{name}_matches_per_pair"] = round(float(c.float().mean()), 1)
        line[f"{name}_exit_layers"] = np.bincount(ex.cpu().numpy(), minlength=9).tolist()
    del ws
    sg_blob = t(pack_superglue_weights(superglue_state_dict(0)))
    ws = torch.empty(L.gtsfm_superglue_workspace_bytes(P, kmax), dtype=torch.uint8, device=dev)
    run = lambda: device.superglue_match(kp, sc, de, cnt, hw, pr, sg_blob, workspace=ws)  # noqa: E731
    run()
    torch.cuda.synchronize()
    line["superglue_ms_per_pair"] = per_pair(windows(run, args.windows), P)
    if args.restatement:
        sd_dev = {key: torch.from_numpy(v).to(dev) for key, v in sd.items()}
        sub = pairs[: args.restatement_pairs]

        def restatement(conf):
            for i, j in sub:
                a, b = planted[i], planted[j]
                lightglue_ref.lightglue(a.kp, b.kp, a.desc, b.desc, a.hw, b.hw, sd_dev, dtype=torch.float32,
                                        depth_confidence=conf, device=dev)

        restatement(-1.0)  # warm-up
        torch.cuda.synchronize()
        reps = max(3, args.windows // 2)
        line["restatement_pairs"] = len(sub)
        line["restatement_full_depth_ms_per_pair"] = per_pair(windows(lambda: restatement(-1.0), reps), len(sub))
        line["restatement_adaptive_ms_per_pair"] = per_pair(windows(lambda: restatement(0.95), reps), len(sub))
    print(json.dumps(line))


if __name__ == "__main__":
    main()
