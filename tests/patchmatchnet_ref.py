"""Torch restatement of PatchmatchNet's eval-mode forward (test infrastructure): the CPU checker of the HIP path, and
the baseline tools/patchmatchnet_bench.py times on the GPU.

Written from the network's behaviour with the reference's fixed configuration; one reference view with its source views
per call, functional over a state dict, in the dtype of its inputs (fp32 or fp64). The random initialisation's uniform
numbers are an argument. Activations are (1, C, H, W); positions are pixel coordinates until the moment of sampling.

The coordinate quirk is kept: the learned grids are normalised as x / ((W - 1) / 2) - 1 but sampled with
align_corners=False and border padding; only the homography warp uses align_corners=True with zero padding.
"""
import numpy as np
import torch
import torch.nn.functional as F

INTERVAL_SCALE = {1: 0.005, 2: 0.0125, 3: 0.025}
PROPAGATION_RANGE = {1: 6, 2: 4, 3: 2}
ITERATIONS = {1: 1, 2: 2, 3: 2}
NUM_SAMPLES = {1: 8, 2: 8, 3: 16}
PROPAGATE_NEIGHBORS = {1: 0, 2: 8, 3: 16}
GROUPS = {1: 4, 2: 8, 3: 8}
INIT_BINS = 48
BN_EPS = 1e-5


def projection_matrices(wRc, wtc, intrinsics):
    """Per-stage 4x4 projection matrices {stage: (n, 4, 4) float64} from camera-to-world poses and (f, u0, v0): the
    first two rows of K divided by 2^stage, times [wRc' | -wRc' wtc]."""
    wRc, wtc, intr = (np.asarray(a, np.float64) for a in (wRc, wtc, intrinsics))
    n = wtc.shape[0]
    out = {}
    for stage in range(4):
        P = np.tile(np.eye(4), (n, 1, 1))
        for i in range(n):
            f, u0, v0 = intr[i]
            K = np.array([[f, 0, u0], [0, f, v0], [0, 0, 1.0]])
            K[:2] /= 2.0 ** stage
            cRw = wRc[i].reshape(3, 3).T
            P[i, :3, :3] = K @ cRw
            P[i, :3, 3] = K @ (-cRw @ wtc[i])
        out[stage] = P
    return out


def _bn(x, sd, name):
    shape = [1, -1] + [1] * (x.dim() - 2)
    scale = sd[f"{name}.weight"] / torch.sqrt(sd[f"{name}.running_var"] + BN_EPS)
    shift = sd[f"{name}.bias"] - sd[f"{name}.running_mean"] * scale
    return x * scale.view(shape) + shift.view(shape)


def _cbr(x, sd, name, stride=1, pad=1):
    return F.relu(_bn(F.conv2d(x, sd[f"{name}.conv.weight"], None, stride, pad), sd, f"{name}.bn"))


def feature_net(sd, img):
    """img (n, 3, H, W) in [0, 1] -> {3: (n, 64, H/8, W/8), 2: (n, 32, H/4, W/4), 1: (n, 16, H/2, W/2)}."""
    p = "feature."
    c1 = _cbr(_cbr(img, sd, p + "conv0"), sd, p + "conv1")
    c4 = _cbr(_cbr(_cbr(c1, sd, p + "conv2", 2, 2), sd, p + "conv3"), sd, p + "conv4")
    c7 = _cbr(_cbr(_cbr(c4, sd, p + "conv5", 2, 2), sd, p + "conv6"), sd, p + "conv7")
    c10 = _cbr(_cbr(_cbr(c7, sd, p + "conv8", 2, 2), sd, p + "conv9"), sd, p + "conv10")
    out = {3: F.conv2d(c10, sd[p + "output1.weight"])}
    intra = F.interpolate(c10, scale_factor=2, mode="bilinear", align_corners=False) + \
        F.conv2d(c7, sd[p + "inner1.weight"], sd[p + "inner1.bias"])
    out[2] = F.conv2d(intra, sd[p + "output2.weight"])
    intra = F.interpolate(intra, scale_factor=2, mode="bilinear", align_corners=False) + \
        F.conv2d(c4, sd[p + "inner2.weight"], sd[p + "inner2.bias"])
    out[1] = F.conv2d(intra, sd[p + "output3.weight"])
    return out


def refinement(sd, img, depth, dmin, dmax):
    """img (1, 3, H, W), depth (1, 1, H/2, W/2) -> (1, 1, H, W)."""
    p = "upsample_net."
    d = (depth - dmin) / (dmax - dmin)
    c0 = _cbr(img, sd, p + "conv0")
    up = F.conv_transpose2d(_cbr(_cbr(d, sd, p + "conv1"), sd, p + "conv2"), sd[p + "deconv.weight"], None, stride=2,
                            padding=1, output_padding=1)
    up = F.relu(_bn(up, sd, p + "bn"))
    res = F.conv2d(_cbr(torch.cat((up, c0), 1), sd, p + "conv3"), sd[p + "res.weight"], None, 1, 1)
    d = F.interpolate(d, scale_factor=2, mode="nearest") + res
    return d * (dmax - dmin) + dmin


def _mlp(x, sd, name, last):
    """The 1x1x1 nets: x (1, G, D, H, W) -> (1, D, H, W) before any sigmoid."""
    for i in (0, 1):
        x = torch.einsum("oc,bcdhw->bodhw", sd[f"{name}.conv{i}.conv.weight"].flatten(1), x)
        x = F.relu(_bn(x, sd, f"{name}.conv{i}.bn"))
    x = torch.einsum("oc,bcdhw->bodhw", sd[f"{name}.{last}.weight"].flatten(1), x)
    return x[:, 0] + sd[f"{name}.{last}.bias"][0]


def _sample_border(x, px, py):
    """x (1, C, H, W) sampled at the pixel positions px, py (N, H, W) with the quirk -> (1, C, N, H, W)."""
    _, C, H, W = x.shape
    N = px.shape[0]
    grid = torch.stack((px / ((W - 1) / 2) - 1, py / ((H - 1) / 2) - 1), dim=-1).view(1, N * H, W, 2)
    return F.grid_sample(x, grid, mode="bilinear", padding_mode="border", align_corners=False).view(1, C, N, H, W)


def _warp(src, rot, trans, samples):
    """src (1, C, H, W) warped to the reference view at samples (1, D, H, W) -> (1, C, D, H, W)."""
    _, C, H, W = src.shape
    D = samples.shape[1]
    ys, xs = torch.meshgrid(torch.arange(H, dtype=src.dtype, device=src.device),
                            torch.arange(W, dtype=src.dtype, device=src.device), indexing="ij")
    xyz = torch.stack((xs.reshape(-1), ys.reshape(-1), torch.ones(H * W, dtype=src.dtype, device=src.device)))
    p = (rot @ xyz)[:, None, :] * samples.view(1, D, H * W) + trans.view(3, 1, 1)
    behind = p[2] <= 1e-3
    px = torch.where(behind, torch.full_like(p[0], W), p[0])
    py = torch.where(behind, torch.full_like(p[1], H), p[1])
    pz = torch.where(behind, torch.ones_like(p[2]), p[2])
    grid = torch.stack(((px / pz) / ((W - 1) / 2) - 1, (py / pz) / ((H - 1) / 2) - 1), dim=-1).view(1, D * H, W, 2)
    return F.grid_sample(src, grid, mode="bilinear", padding_mode="zeros", align_corners=True).view(1, C, D, H, W)


def _offset_positions(base, offset, H, W):
    """Pixel positions of the neighbours: base [(dy, dx)], offset (1, 2N, H, W) with channel 2i = x, 2i + 1 = y."""
    ys, xs = torch.meshgrid(torch.arange(H, dtype=offset.dtype, device=offset.device),
                            torch.arange(W, dtype=offset.dtype, device=offset.device), indexing="ij")
    px = torch.stack([xs + (dx + offset[0, 2 * i]) for i, (dy, dx) in enumerate(base)])
    py = torch.stack([ys + (dy + offset[0, 2 * i + 1]) for i, (dy, dx) in enumerate(base)])
    return px, py


def propagation_offsets(stage):
    d = PROPAGATION_RANGE[stage]
    ring = [(-d, -d), (-d, 0), (-d, d), (0, -d), (0, d), (d, -d), (d, 0), (d, d)]
    if PROPAGATE_NEIGHBORS[stage] == 16:
        ring = ring + [(2 * a, 2 * b) for a, b in ring]
    return ring if PROPAGATE_NEIGHBORS[stage] else []


def evaluation_offsets(stage):
    d = PROPAGATION_RANGE[stage] - 1
    return [(a * d, b * d) for a in (-1, 0, 1) for b in (-1, 0, 1)]


def patchmatch_stage(sd, stage, ref, srcs, rots, transs, dmin, dmax, depth, view_weights, uniform, iter_depths):
    """One stage for one reference view. ref (1, C, H, W), srcs a list of the same, rots / transs the 3x3 and 3 parts
    of src_proj ref_proj^-1, depth (1, 1, H, W) or None on stage 3, view_weights (1, S, H, W) or None on stage 3.
    Returns (depth (1, 1, H, W), score (1, D, H, W), view_weights)."""
    p = f"patchmatch_{stage}"
    _, C, H, W = ref.shape
    G, dil, Ns, scale = GROUPS[stage], PROPAGATION_RANGE[stage], NUM_SAMPLES[stage], INTERVAL_SCALE[stage]
    if PROPAGATE_NEIGHBORS[stage]:
        off = F.conv2d(ref, sd[p + ".propa_conv.weight"], sd[p + ".propa_conv.bias"], 1, dil, dil)
        ppx, ppy = _offset_positions(propagation_offsets(stage), off, H, W)
    off = F.conv2d(ref, sd[p + ".eval_conv.weight"], sd[p + ".eval_conv.bias"], 1, dil, dil)
    epx, epy = _offset_positions(evaluation_offsets(stage), off, H, W)
    ref_g = ref.view(1, G, C // G, 1, H, W)
    corr = (_sample_border(ref, epx, epy).view(1, G, C // G, 9, H, W) * ref_g).mean(2)
    feature_weight = torch.sigmoid(_mlp(corr, sd, p + ".feature_weight_net", "similarity"))  # (1, 9, H, W)
    inv_min, inv_max = 1.0 / dmin, 1.0 / dmax
    score = None
    for it in range(1, ITERATIONS[stage] + 1):
        if depth is None:
            k = torch.arange(INIT_BINS, dtype=ref.dtype, device=ref.device).view(1, -1, 1, 1)
            samples = 1.0 / (inv_max + (uniform.view(1, INIT_BINS, H, W) + k) / INIT_BINS * (inv_min - inv_max))
        else:
            k = torch.arange(-Ns // 2, Ns // 2, dtype=ref.dtype, device=ref.device).view(1, -1, 1, 1)
            inv = 1.0 / depth + (inv_min - inv_max) * scale * k
            samples = 1.0 / torch.clamp(inv, min=inv_max, max=inv_min)
            if PROPAGATE_NEIGHBORS[stage]:
                prop = _sample_border(samples[:, Ns // 2: Ns // 2 + 1], ppx, ppy)[:, 0]
                samples = torch.sort(torch.cat((samples, prop), 1), dim=1)[0]
        D = samples.shape[1]
        xn = (1.0 / samples - inv_max) / (inv_min - inv_max)
        diff = torch.abs(_sample_border(xn, epx, epy) - xn[:, :, None]) / scale
        weight = torch.sigmoid((2 - torch.clamp(diff, 0, 4)) * 2) * feature_weight[:, None]
        weight = weight / weight.sum(2, keepdim=True)                                        # (1, D, 9, H, W)
        sim_sum, w_sum, new_weights = 0, 0, []
        for i, (src, rot, trans) in enumerate(zip(srcs, rots, transs)):
            sim = (_warp(src, rot, trans, samples).view(1, G, C // G, D, H, W) * ref_g).mean(2)
            if view_weights is None:
                w = torch.sigmoid(_mlp(sim, sd, p + ".evaluation.pixel_wise_net", "conv2")).max(1)[0][:, None]
                new_weights.append(w)
            else:
                w = view_weights[:, i: i + 1]
            sim_sum = sim_sum + sim * w[:, None]
            w_sum = w_sum + w[:, None]
        if view_weights is None:
            view_weights = torch.cat(new_weights, 1)
        cost = _mlp(sim_sum / w_sum, sd, p + ".evaluation.similarity_net", "similarity")     # (1, D, H, W)
        score = torch.softmax((_sample_border(cost, epx, epy) * weight).sum(2), dim=1)
        if stage == 1 and it == ITERATIONS[stage]:
            index = (torch.arange(D, dtype=ref.dtype, device=ref.device).view(1, -1, 1, 1) * score).sum(1)
            inv_far, inv_near = 1.0 / samples[:, 0], 1.0 / samples[:, -1]
            depth = 1.0 / (inv_far + index / (D - 1) * (inv_near - inv_far))
        else:
            depth = (samples * score).sum(1)
        depth = depth[:, None]
        iter_depths.append(depth)
    return depth, score, view_weights


def confidence_from_score(score):
    """score (1, 8, H, W) of stage 1 -> (1, 2H, 2W): the sum of four neighbouring probabilities at the regressed
    index; also returns the regression index (1, H, W) before truncation."""
    D = score.shape[1]
    padded = F.pad(score, (0, 0, 0, 0, 1, 2))
    sum4 = sum(padded[:, j: j + D] for j in range(4))
    index = (torch.arange(D, dtype=score.dtype, device=score.device).view(1, -1, 1, 1) * score).sum(1)
    pick = torch.clamp(index.long(), 0, D - 1)
    conf = torch.gather(sum4, 1, pick[:, None])
    return F.interpolate(conf, scale_factor=2, mode="nearest")[:, 0], index


def patchmatchnet_forward(sd, images, projs, depth_min, depth_max, uniform, features=None):
    """images (V, 3, H, W) in [0, 1], the reference view first; projs {stage: (V, 4, 4)}; uniform (48, H/8, W/8). All
    in one dtype, which sd shares. features: feature_net's result for the V images if already computed. Returns a dict:
    depth (H, W), confidence (H, W), features {stage: (V, C, h, w)}, iter_depths (five (h, w) maps), index (H/2, W/2)."""
    if features is None:
        features = feature_net(sd, images)
    V = images.shape[0]
    depth, view_weights, score, iter_depths = None, None, None, []
    for stage in (3, 2, 1):
        fea = features[stage]
        proj = projs[stage]
        rel = [proj[i] @ torch.inverse(proj[0]) for i in range(1, V)]
        depth, score, view_weights = patchmatch_stage(
            sd, stage, fea[:1], [fea[i: i + 1] for i in range(1, V)], [r[:3, :3] for r in rel],
            [r[:3, 3] for r in rel], depth_min, depth_max, depth, view_weights, uniform, iter_depths)
        if stage > 1:
            depth = F.interpolate(depth, scale_factor=2, mode="nearest")
            view_weights = F.interpolate(view_weights, scale_factor=2, mode="nearest")
    refined = refinement(sd, images[:1], depth, depth_min, depth_max)
    conf, index = confidence_from_score(score)
    return {"depth": refined[0, 0], "confidence": conf[0], "features": features,
            "iter_depths": [d[0, 0] for d in iter_depths], "index": index[0]}


def torch_state_dict(sd_np, dtype, device="cpu"):
    """The numpy state dict as torch tensors of dtype (the integer BatchNorm counters are dropped)."""
    return {k: torch.from_numpy(np.asarray(v)).to(device=device, dtype=dtype) for k, v in sd_np.items()
            if not k.endswith("num_batches_tracked")}


def load_golden_case(z, name):
    """The inputs and recorded outputs of one case of tests/golden/patchmatchnet_random_w0.npz as a dict."""
    prefix = f"{name}__"
    return {k[len(prefix):]: z[k] for k in z.files if k.startswith(prefix)}


def batch_uniform(case, seed=1):
    """Uniform numbers (n, 48, H/8, W/8) float32 for every view of a case: the golden's for view 0, seeded for the
    rest."""
    n, H, W = case["images"].shape[:3]
    u = np.random.default_rng(seed).uniform(0, 1, (n, INIT_BINS, H // 8, W // 8)).astype(np.float32)
    u[0] = case["uniform"]
    return u


def run_case(sd_np, case, dtype, ref_view=0, uniform=None, device="cpu"):
    """patchmatchnet_forward for one reference view of a golden case and its source views."""
    views = [ref_view] + [int(s) for s in case["src_views"][ref_view]]
    projs = projection_matrices(case["wRc"][views], case["wtc"][views], case["intrinsics"][views])
    sd = torch_state_dict(sd_np, dtype, device)
    img = torch.from_numpy(case["images"][views].astype(np.float32) / 255.0).permute(0, 3, 1, 2).to(device, dtype)
    P = {s: torch.from_numpy(p).to(device, dtype) for s, p in projs.items()}
    dmin, dmax = (torch.tensor(case["depth_range"][ref_view, k], dtype=dtype, device=device) for k in (0, 1))
    u = torch.from_numpy(case["uniform"] if uniform is None else uniform).to(device, dtype)
    with torch.no_grad():
        return patchmatchnet_forward(sd, img, P, dmin, dmax, u)


def error_figures(value, exact, span):
    """(median, 99th percentile, share above 1e-4 of span) of |value - exact|."""
    err = np.abs(np.asarray(value, np.float64) - np.asarray(exact, np.float64)).ravel()
    return float(np.median(err)), float(np.percentile(err, 99)), float((err > 1e-4 * span).mean())
