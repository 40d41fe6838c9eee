#!/usr/bin/env python
"""D2-Net detection and description (gtsfm_d2net_batched) timed on the MI355X with HIP events after warm-up: the whole
call, and its stages from calls stopped after each one (gtsfm_d2net_stages): trunk (preprocessing, conv1_1 .. conv3_3,
average pool), the three dilated convolutions, detection with the candidate list and the top-k, description.
--restatement also times tests/d2net_ref.py under torch-ROCm in fp32 on the same GPU and the same images, one image at
a time as the reference runs, and reports the ratio.

    python tools/d2net_bench.py --images 8 --height 1200 --width 1600 --max-keypoints 5000 --restatement
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
from gtsfm_amd.frontend.detector_descriptor.d2net import pack_d2net_weights  # noqa: E402

STAGES = ("trunk", "dilated", "detect", "describe")


def timed(fn, repeats):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(repeats):
        start.record()
        fn()
        stop.record()
        torch.cuda.synchronize()
        out.append(start.elapsed_time(stop))
    return float(np.median(out))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--max-keypoints", type=int, default=5000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--restatement", action="store_true")
    args = ap.parse_args()
    native.require_gpu()
    from d2net_weights import d2net_state_dict, textured_image

    n, H, W, k = args.images, args.height, args.width, args.max_keypoints
    dev = torch.device("cuda:0")
    sd = d2net_state_dict(0)
    arrays = [textured_image(args.seed + i, H, W) for i in range(n)]
    images = torch.from_numpy(np.stack(arrays)).to(dev)
    blob = torch.from_numpy(pack_d2net_weights(sd)).to(dev)
    L = native.lib()
    ws = torch.empty(L.gtsfm_d2net_workspace_bytes(n, H, W, k), dtype=torch.uint8, device=dev)
    out = device.d2net_extract(images, blob, k, workspace=ws)  # warm-up: code objects, first launches
    torch.cuda.synchronize()
    call_ms = timed(lambda: device.d2net_extract(images, blob, k, workspace=ws, out=out), args.repeats)
    upto = [timed(lambda s=s: device.d2net_extract(images, blob, k, workspace=ws, out=out, last_stage=s), args.repeats)
            for s in range(4)]
    stage = [upto[0]] + [upto[i] - upto[i - 1] for i in range(1, 4)]
    h, w = device.d2net_map_shape(H, W)
    dil_flop = 2.0 * 9 * (256 * 512 + 2 * 512 * 512) * h * w * n
    line = {"tool": "d2net_bench", "images": n, "height": H, "width": W, "max_keypoints": k, "map": [h, w],
            "workspace_MiB": round(ws.numel() / 2 ** 20, 1), "call_ms": round(call_ms, 3),
            "per_image_ms": round(call_ms / n, 3), "stage_ms": {s: round(v, 3) for s, v in zip(STAGES, stage)},
            "dilated_share": round(stage[1] / upto[3], 4),
            "dilated_TFLOPs_fp32_equivalent": round(dil_flop / (stage[1] * 1e-3) / 1e12, 2),
            "keypoints": out.count.cpu().tolist(), "candidates": out.n_candidates.cpu().tolist()}
    if args.restatement:
        import d2net_ref as dref

        sd_dev = {key: torch.from_numpy(v).to(dev) for key, v in sd.items()}
        got = dref.run(sd_dev, arrays[0], torch.float32, k, device=dev)  # warm-up
        torch.cuda.synchronize()

        def restatement():
            for a in arrays:
                dref.run(sd_dev, a, torch.float32, k, device=dev)

        ref_ms = timed(restatement, max(1, args.repeats // 2))
        m = min(len(got["scores"]), int(out.count[0]))
        line.update(restatement_ms=round(ref_ms, 3), restatement_per_image_ms=round(ref_ms / n, 3),
                    speedup=round(ref_ms / call_ms, 2), restatement_keypoints_image0=len(got["scores"]),
                    top_score_diff_image0=float(np.abs(got["scores"][:m] - out.scores[0, :m].cpu().numpy()).max())
                    if m else None)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
