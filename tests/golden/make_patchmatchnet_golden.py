"""Golden PatchmatchNet outputs from the reference's own module (run in the build container, where /root/reference
exists; the GPU box has no reference and only reads the .npz this writes).

thirdparty/patchmatchnet/models/net.py is imported as-is, loaded with the seeded weights of
tests/patchmatchnet_weights.py (regenerated from the seed by the tests, not stored: see that module) and run on the CPU
twice per case: in fp32, and after .double() with every input in fp64. For the second run torch.rand returns the same
uniform numbers and Tensor.float is a cast to fp64, because the module narrows its projection matrices and depth range
with .float() whatever its own dtype: without that the "fp64" run would share the fp32 run's matrix inverse.

Per case the npz holds the inputs of the whole batch (images, poses, intrinsics, source views, depth ranges), the
uniform numbers of view 0 and, for view 0 as the reference view: refined depth, confidence, the five per-iteration
depths and the stage-1 regression index in fp32 and fp64, and view 0's three feature maps (the fp64 run's, stored as
fp32, which is 1e-7 against a 2e-4 check).

A second file, patchmatchnet_edges_w0.npz, ties the restatement to the module on the shapes of
tests/patchmatchnet_cases.py: for every view of cases (c) and (d) as the reference view, with its valid sources in row
order and the batch's uniform numbers, the fp64 run's stage-1 depth (iter4), regression index and confidence at half
resolution ([::2, ::2]: the full map is its x2 nearest copy), as float64. The inputs are not stored: the tests rebuild
them from the seed.

    python tests/golden/make_patchmatchnet_golden.py [gain]
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, REF)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(HERE))  # tests/ (the reference has a `tests` package of its own)

import patchmatchnet_cases as pcases  # noqa: E402
import patchmatchnet_ref as pref  # noqa: E402
from patchmatchnet_weights import GAIN, patchmatchnet_state_dict  # noqa: E402


def _rot(yaw, pitch, roll):
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    Rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    return Ry @ Rx @ Rz


def _images(rng, V, H, W):
    """Smooth images that correlate between the views: one low-resolution noise field upsampled, shifted by a few
    pixels per view, plus a little per-view noise."""
    low = torch.from_numpy(rng.uniform(0, 1, (1, 3, H // 8 + 4, W // 8 + 4)))
    big = F.interpolate(low, size=(H + 32, W + 32), mode="bicubic", align_corners=False)[0].numpy()
    out = np.zeros((V, H, W, 3), np.uint8)
    for v in range(V):
        dy, dx = rng.integers(0, 12, 2)
        crop = big[:, 8 + dy: 8 + dy + H, 8 + dx: 8 + dx + W].transpose(1, 2, 0)
        out[v] = np.clip((crop + rng.normal(0, 0.02, crop.shape)) * 255.0, 0, 255).astype(np.uint8)
    return out


def cases(seed=0):
    rng = np.random.default_rng(seed)
    out = {}
    # (a) 72 x 104, 3 views: stage maps 36 x 52, 18 x 26, 9 x 13
    V, H, W = 3, 72, 104
    wtc = np.array([[0.0, 0.0, 0.0], [0.25, 0.02, 0.0], [-0.2, 0.05, 0.05]])
    wRc = np.stack([_rot(0, 0, 0), _rot(-0.03, 0.01, 0.02), _rot(0.04, -0.02, -0.01)])
    out["a"] = dict(images=_images(rng, V, H, W), wRc=wRc, wtc=wtc,
                    intrinsics=np.tile(np.array([110.0, 52.0, 36.0]), (V, 1)),
                    src_views=np.array([[1, 2], [0, 2], [0, 1]], np.int32),
                    depth_range=np.tile(np.array([2.5, 6.0]), (V, 1)))
    # (b) 64 x 80, 5 views, unequal intrinsics and depth ranges; view 4 stands inside view 0's depth range and looks
    # sideways, so part of view 0's hypotheses fall behind it and part project outside its image
    V, H, W = 5, 64, 80
    wtc = np.array([[0.0, 0.0, 0.0], [0.2, 0.0, 0.02], [-0.15, 0.06, 0.0], [0.05, -0.18, -0.04], [0.3, 0.0, 3.2]])
    wRc = np.stack([_rot(0, 0, 0), _rot(-0.04, 0.0, 0.01), _rot(0.03, 0.02, 0.0), _rot(0.01, -0.04, -0.02),
                    _rot(-1.4, 0.05, 0.0)])
    intr = np.array([[90.0, 40.0, 32.0], [86.0, 41.5, 31.0], [95.0, 38.5, 33.0], [100.0, 40.5, 30.5],
                     [88.0, 39.0, 32.5]])
    rows = np.array([[j for j in range(V) if j != i] for i in range(V)], np.int32)
    out["b"] = dict(images=_images(rng, V, H, W), wRc=wRc, wtc=wtc, intrinsics=intr, src_views=rows,
                    depth_range=np.array([[2.0, 5.0], [2.2, 5.5], [1.8, 4.5], [2.0, 6.0], [1.5, 4.0]]))
    for c in out.values():
        H, W = c["images"].shape[1:3]
        c["uniform"] = rng.uniform(0, 1, (pref.INIT_BINS, H // 8, W // 8)).astype(np.float32)
    return out


def reference_model(sd_np, dtype):
    from thirdparty.patchmatchnet.models.net import PatchmatchNet

    model = PatchmatchNet()
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd_np.items()}, strict=True)
    return model.to(dtype).eval()


def run_reference(model, case, dtype, ref_view=0, uniform=None):
    """uniform: the (48, H/8, W/8) numbers of ref_view; the default is the case's own (view 0's). Source indices
    outside the batch are left out, as the kernels skip them."""
    n = case["images"].shape[0]
    views = [ref_view] + [int(s) for s in case["src_views"][ref_view] if 0 <= s < n]
    img = torch.from_numpy(case["images"][views].astype(np.float32) / 255.0).permute(0, 3, 1, 2).to(dtype)
    projs = pref.projection_matrices(case["wRc"][views], case["wtc"][views], case["intrinsics"][views])
    imgs = {f"stage_{s}": img[None, :, :, ::2 ** s, ::2 ** s] for s in range(4)}  # only stage_0 is read
    proj = {f"stage_{s}": torch.from_numpy(projs[s])[None].to(dtype) for s in range(4)}
    dmin, dmax = (torch.tensor([case["depth_range"][ref_view, k]], dtype=dtype) for k in (0, 1))
    uniform = torch.from_numpy(case["uniform"] if uniform is None else uniform)[None].to(dtype)
    grabbed = {}

    def keep_features(module, args, output):  # called once per view, the reference view first (a hook returns None)
        grabbed.setdefault("features", output)

    def keep_score(module, args, output):
        grabbed["score"] = output[1]

    hooks = [model.feature.register_forward_hook(keep_features), model.patchmatch_1.register_forward_hook(keep_score)]
    real_rand, real_float, real_arange = torch.rand, torch.Tensor.float, torch.arange
    torch.rand = lambda *a, **k: uniform.clone()
    if dtype == torch.float64:
        torch.Tensor.float = lambda self: self.double()
        # the pixel grids are built with dtype=torch.float32 spelled out; the integers are exact in either type
        torch.arange = lambda *a, **k: real_arange(*a, **{**k, "dtype": dtype} if k.get("dtype") == torch.float32
                                                   else k)
    try:
        with torch.no_grad():
            out = model(imgs, proj, dmin, dmax)
    finally:
        torch.rand, torch.Tensor.float, torch.arange = real_rand, real_float, real_arange
        for h in hooks:
            h.remove()
    iters = [d[0, 0] for s in (3, 2, 1) for d in out["depth_patchmatch"][f"stage_{s}"]]
    score = grabbed["score"]
    index = (torch.arange(score.shape[1], dtype=dtype).view(1, -1, 1, 1) * score).sum(1)[0]
    res = {"depth": out["refined_depth"]["stage_0"][0, 0], "confidence": out["photometric_confidence"][0],
           "index": index}
    res.update({f"iter{i}": d for i, d in enumerate(iters)})
    res.update({f"feat{s}": grabbed["features"][f"stage_{s}"][0] for s in (1, 2, 3)})
    return {k: v.numpy() for k, v in res.items()}


def nondegeneracy(r32, r64, depth_range):
    """The three conditions on the golden: confidence std, share of pixels with a near-integer regression index, share
    of pixels where the fp32 run strays from the fp64 run by more than 1e-4 of the depth range."""
    span = depth_range[1] - depth_range[0]
    near = np.abs(r64["index"] - np.round(r64["index"])) < 1e-3
    return (float(r64["confidence"].std()), float(near.mean()),
            float((np.abs(r32["depth"] - r64["depth"]) > 1e-4 * span).mean()))


def main():
    gain = float(sys.argv[1]) if len(sys.argv) > 1 else GAIN
    sd = patchmatchnet_state_dict(0, gain)
    m32, m64 = reference_model(sd, torch.float32), reference_model(sd, torch.float64)
    res = {"gain": np.array(gain), "torch_version": np.array(torch.__version__)}
    for name, case in cases().items():
        r32, r64 = run_reference(m32, case, torch.float32), run_reference(m64, case, torch.float64)
        std, near, stray = nondegeneracy(r32, r64, case["depth_range"][0])
        err = np.abs(r32["depth"] - r64["depth"])
        print(f"case {name}: gain {gain} confidence std {std:.4f} near-integer index {near:.4%} fp32 beyond 1e-4 "
              f"{stray:.4%} fp32 depth error median {np.median(err):.3g} p99 {np.percentile(err, 99):.3g} max "
              f"{err.max():.3g}")
        for k, v in case.items():
            res[f"{name}__{k}"] = v
        for k in r64:
            if k.startswith("feat"):
                res[f"{name}__{k}"] = r64[k].astype(np.float32)
            else:
                res[f"{name}__{k}_f32"] = r32[k].astype(np.float32)
                res[f"{name}__{k}_f64"] = r64[k].astype(np.float64)
    path = os.path.join(HERE, "patchmatchnet_random_w0.npz")
    np.savez_compressed(path, **res)
    print(path, os.path.getsize(path), "bytes")
    edges = {"gain": np.array(gain), "torch_version": np.array(torch.__version__)}
    for name, case in pcases.cases().items():
        uniform = pref.batch_uniform(case)
        for v in range(case["images"].shape[0]):
            r64 = run_reference(m64, case, torch.float64, ref_view=v, uniform=uniform[v])
            edges[f"{name}__view{v}__iter4"] = r64["iter4"].astype(np.float64)
            edges[f"{name}__view{v}__index"] = r64["index"].astype(np.float64)
            edges[f"{name}__view{v}__confidence_half"] = r64["confidence"][::2, ::2].astype(np.float64)
            print(f"case {name} view {v}: confidence std {r64['confidence'].std():.4f}")
    path = os.path.join(HERE, "patchmatchnet_edges_w0.npz")
    np.savez_compressed(path, **edges)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
