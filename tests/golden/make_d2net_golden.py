"""Golden D2-Net outputs from the reference's own modules (run where a checkout of the reference exists, as
tests/golden/make_patchmatchnet_golden.py; the tests only read the .npz this writes).

thirdparty/d2net/lib/model_test.py (D2Net) and pyramid.py (process_multiscale) are imported as-is, loaded with the
seeded weights of tests/d2net_weights.py (regenerated from the seed by the tests, not stored) and run on the CPU with
scales = [1], in fp32 and after .double() (the detection and localisation filters are plain tensors, so they are
widened by hand). Two images of tests/d2net_weights.textured_image: `a` RGB 48 x 64, `b` gray 52 x 44 repeated to three
channels.

Per image the npz holds: the uint8 image; the dense map of the fp64 run stored as fp32; process_multiscale's outputs
in its own (candidate) order for both runs: keypoints (N, 2) = (i, j) in image pixels and scores as fp64 / fp32, and
the descriptors of every DESC_STRIDE-th keypoint (desc_rows), which keeps the file within the limit for a committed
file. The maker asserts the non-degeneracy that tests/test_d2net_ref.py checks again.

A second file, d2net_planted_ties.npz, pins exact channel ties (tests/test_d2net_planted.py): the pass-through weights
of tests/d2net_planted.py with channels 300 and 301 exact copies of channels 0 and 1, in the same D2Net module on a
4 x 4-block noise image with a 17 x 33 map, fp32. It holds the image and process_multiscale's keypoints (i, j) and
scores in its own order, with the channel of every row: the detected channels of a location (the module's own
detection mask) in ascending order, one per row of that location, which is torch.nonzero's order. No dense map.

    python tests/golden/make_d2net_golden.py [random] [planted]
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, REF)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(HERE))  # tests/ (the reference has a `tests` package of its own)

import d2net_planted as dplant  # noqa: E402
import d2net_ref as dref  # noqa: E402
from d2net_weights import d2net_state_dict, textured_image  # noqa: E402

DESC_STRIDE = 6
# image seeds: the first of 1, 2, ... whose image has a detection rejected by each of the three later tests
CASES = {"a": dict(seed=2, H=48, W=64, gray=False), "b": dict(seed=15, H=52, W=44, gray=True)}
PLANTED = dict(seed=2, H4=18, W4=34)  # block grid of the planted tie case


def reference_model(sd_np, dtype):
    from thirdparty.d2net.lib.model_test import D2Net

    model = D2Net(model_file=None, use_relu=True, use_cuda=False)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd_np.items()}, strict=True)
    model = model.to(dtype).eval()
    for mod in (model.detection, model.localization):
        for name, val in list(vars(mod).items()):
            if name.endswith("_filter"):
                setattr(mod, name, val.to(dtype))
    return model


def run_reference(model, image, dtype):
    from thirdparty.d2net.lib.pyramid import process_multiscale

    x = torch.from_numpy(dref.preprocess(image))[None].to(dtype)
    with torch.no_grad():
        kp, scores, desc = process_multiscale(x, model, scales=[1])
        dense = model.dense_feature_extraction(x)[0].numpy()
    return dict(dense=dense, kp=kp[:, :2], scores=scores, desc=desc)


def main():
    sd = d2net_state_dict(0)
    m32, m64 = reference_model(sd, torch.float32), reference_model(sd, torch.float64)
    res = {"torch_version": np.array(torch.__version__), "desc_stride": np.array(DESC_STRIDE)}
    for name, c in CASES.items():
        image = textured_image(c["seed"], c["H"], c["W"], c["gray"])
        r32, r64 = run_reference(m32, image, torch.float32), run_reference(m64, image, torch.float64)
        assert r64["dense"].dtype == np.float64 and r64["kp"].dtype == np.float64, (r64["dense"].dtype, r64["kp"].dtype)
        mine = dref.run(sd, image, torch.float64)
        rej = [mine[k] for k in ("rejected_edge", "rejected_step", "rejected_corner")]
        sat = float((r64["dense"] > 0).mean())
        print(f"case {name}: map {r64['dense'].shape} max {r64['dense'].max():.4g} positive share {sat:.3f}; "
              f"{len(r64['scores'])} keypoints (fp32 run {len(r32['scores'])}); rejected by edge / step / corner {rej}")
        assert len(r64["scores"]) >= 50, "fewer than 50 keypoints"
        assert min(rej) >= 1, "a rejection path is not exercised: change the image"
        assert 0.05 < sat < 0.95, "map all zero or saturated"
        rows = np.arange(0, len(r64["scores"]), DESC_STRIDE)
        res[f"{name}__image"] = image
        res[f"{name}__dense"] = r64["dense"].astype(np.float32)
        res[f"{name}__desc_rows"] = rows
        for tag, r, dt in (("f64", r64, np.float64), ("f32", r32, np.float32)):
            res[f"{name}__kp_{tag}"] = r["kp"].astype(dt)
            res[f"{name}__scores_{tag}"] = r["scores"].astype(dt)
            res[f"{name}__desc_{tag}"] = r["desc"][np.arange(0, len(r["scores"]), DESC_STRIDE)].astype(dt)
    path = os.path.join(HERE, "d2net_random_w0.npz")
    np.savez_compressed(path, **res)
    print(path, os.path.getsize(path), "bytes")


def main_planted():
    u = dplant.noise_blocks(PLANTED["seed"], PLANTED["H4"], PLANTED["W4"])
    image = dplant.block_image(u)
    model = reference_model(dplant.passthrough_state_dict(dplant.channel_sources(), dplant.tie_gains()), torch.float32)
    r = run_reference(model, image, torch.float32)
    with torch.no_grad():
        detected = model.detection(torch.from_numpy(r["dense"])[None])[0].numpy()
    ij = np.round((r["kp"].astype(np.float64) - 1.5) / 4).astype(np.int64)
    seen, chan = {}, []
    for i, j in ij.tolist():
        cs = np.flatnonzero(detected[:, i, j])
        q = seen.get((i, j), 0)
        assert q < len(cs), "more rows at a location than detected channels"
        chan.append(cs[q])
        seen[(i, j)] = q + 1
    cij = np.concatenate([np.array(chan)[:, None], ij], axis=1)
    # every detected channel of a kept location is listed, rows are in torch.nonzero order, a score is its map value
    assert all(n == int(detected[:, i, j].sum()) for (i, j), n in seen.items())
    assert np.all(np.lexsort((cij[:, 2], cij[:, 1], cij[:, 0])) == np.arange(len(cij)))
    assert np.array_equal(r["dense"][cij[:, 0], cij[:, 1], cij[:, 2]], r["scores"])
    tied = sum(n > 1 for n in seen.values())
    print(f"planted: map {r['dense'].shape}, {len(cij)} keypoints in channels {sorted(set(chan))}, {tied} tied pairs")
    assert tied >= 20 and set(chan) == set(dplant.TIE_CHANNELS)
    path = os.path.join(HERE, "d2net_planted_ties.npz")
    np.savez_compressed(path, torch_version=np.array(torch.__version__), image=image, cij=cij.astype(np.int32),
                        kp=r["kp"].astype(np.float32), scores=r["scores"].astype(np.float32))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    which = sys.argv[1:] or ["random", "planted"]
    if "random" in which:
        main()
    if "planted" in which:
        main_planted()
