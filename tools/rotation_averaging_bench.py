"""Times Shonan rotation averaging (gtsfm_rotavg_shonan) on a synthetic scene: --images cameras with random rotations,
--edge-frac of the pairs as edges plus a spanning chain, relative rotations disturbed by --noise-deg.

    python tools/rotation_averaging_bench.py [--restatement]

Prints one JSON line: time per call (median of --repeats), the levels visited, lambda_min and its residual, the LM /
PCG / Lanczos counts and the number of Out = V Q products they imply. The products are not timed on their own: that
needs a kernel profile of the call. With --restatement the numpy restatement (tests/rotation_averaging_ref.py) solves
the same scene on the CPU; its time is reported next to the GPU's, not a target, and the two results are compared.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def scene(n, frac, noise_deg, seed):
    from tests import rotation_averaging_ref as ref

    rng = np.random.default_rng(seed)
    wRi = np.array([ref.rodrigues(rng.normal(size=3)) for _ in range(n)])
    iu = np.triu_indices(n, 1)
    pick = rng.random(len(iu[0])) < frac
    pick |= (iu[1] - iu[0]) == 1
    i1, i2 = iu[0][pick], iu[1][pick]
    noise = np.array([ref.rodrigues(np.deg2rad(noise_deg) * w / np.sqrt(3.0)) for w in rng.normal(size=(len(i1), 3))])
    i2Ri1 = np.einsum("eji,ejk,ekl->eil", wRi[i2], wRi[i1], noise)
    return wRi, np.stack([i1, i2], 1).astype(np.int32), i2Ri1


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--edge-frac", type=float, default=0.03)
    ap.add_argument("--noise-deg", type=float, default=3.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--restatement", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from gtsfm_amd import device, native
    from tests import rotation_averaging_ref as ref

    native.require_gpu()
    dev = torch.device("cuda:0")
    wRi, pairs, i2Ri1 = scene(args.images, args.edge_frac, args.noise_deg, args.seed)
    ab = torch.from_numpy(np.ascontiguousarray(pairs[:, ::-1])).to(dev)
    R = torch.from_numpy(np.ascontiguousarray(i2Ri1)).to(dev)
    need = native.lib().gtsfm_rotavg_workspace_bytes(len(pairs), args.images, 30)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    times = []
    for _ in range(args.repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = device.rotavg_shonan(ab, R, None, None, args.images, seed=args.seed, workspace=ws)
        times.append(time.perf_counter() - t0)  # the call synchronises its stream
    stats = dict(zip(native.RA_STATS_FIELDS, res.stats.cpu().numpy().tolist()))
    got = res.wRi.cpu().numpy()
    line = {"images": args.images, "edges": len(pairs), "workspace_mib": round(need / 2 ** 20, 1),
            "ms_per_call": round(1e3 * float(np.median(times[1:])), 2), "levels_visited": int(stats["final_p"]) - 5 + 1,
            "products": int(stats["pcg_iterations"] + stats["lanczos_steps"] + 2 * stats["lm_iterations"]),
            "max_error_to_truth_deg": float(ref.aligned_angles_deg(wRi, got, res.rot_valid.cpu().numpy()).max()), **stats}
    if args.restatement:
        edges, aRb, kappa = ref.edges_from_two_view(pairs, i2Ri1)
        t0 = time.perf_counter()
        want = ref.shonan(edges, aRb, kappa, None, args.images, seed=args.seed)
        line["restatement_s"] = round(time.perf_counter() - t0, 2)
        line["restatement_final_p"] = want.stats[2]
        line["restatement_lambda_min"] = want.stats[3]
        line["max_difference_deg"] = float(ref.aligned_angles_deg(want.wRi, got, want.rot_valid).max())
        line["cost_difference"] = abs(want.stats[1] - stats["final_cost"])
    line = json.dumps(line)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
