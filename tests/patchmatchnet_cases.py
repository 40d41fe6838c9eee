"""PatchmatchNet cases (c) and (d) (test infrastructure): the shapes the golden's cases (a) and (b) do not reach, built
from a seed in numpy alone, with elementwise IEEE arithmetic only (no interpolation routine, no matrix product, no
trigonometry), so the bytes are the same on every machine. The weights are those of the golden:
patchmatchnet_state_dict(0) at its gain. The expectation of a view is tests/patchmatchnet_ref.py in fp64 with that
view's valid sources in row order; tests/golden/patchmatchnet_edges_w0.npz ties that to the reference's own module.

(c) minimum, 16 x 24, 2 views, 1 source each: stage maps 8 x 12, 4 x 6 and 2 x 3 (not square: a swapped H and W shows).
    On the 2 x 3 map every propagation neighbour (+-2, +-4) and every evaluation neighbour lies outside the map and
    the border rule divides by (size - 1) / 2 = 0.5. Its confidence is uniform (std about 0): the subject of this case
    is the features and the five iteration depths at the clamped borders, not the confidence.
(d) seams, 136 x 152, 3 views, n_src = 3 with ragged rows: stage maps 17 x 19, 34 x 38 and 68 x 76 under the full
    136 x 152, so every level has a full 16 x 16 tile plus a remainder tile of 1, 2, 4 and 8 rows and of 3, 6, 12 and
    8 columns. Row 0 ends in -1, row 1 starts with -1 (its first valid source is not slot 0), row 2 holds an index
    >= n_views. Intrinsics and depth ranges differ per view.
"""
import numpy as np

import patchmatchnet_ref as pref

SEEDS = {"c": 11, "d": 12}


def _rot(a, b, c):
    """The rotation of the quaternion (1, a, b, c) / norm: square root and division only."""
    q = np.array([1.0, a, b, c])
    w, x, y, z = q / np.sqrt((q * q).sum())
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _cubic_axis(a, axis, n_out):
    """Catmull-Rom resampling of one axis to n_out samples (pixel centres aligned, indices clamped at the ends)."""
    n_in = a.shape[axis]
    pos = (np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5
    base = np.floor(pos)
    t = pos - base
    weights = (((-0.5 * t + 1.0) * t - 0.5) * t, (1.5 * t - 2.5) * t * t + 1.0, ((-1.5 * t + 2.0) * t + 0.5) * t,
               (0.5 * t - 0.5) * t * t)
    shape = [1] * a.ndim
    shape[axis] = n_out
    out = 0.0
    for k, wk in enumerate(weights):
        idx = np.clip(base.astype(np.int64) + (k - 1), 0, n_in - 1)
        out = out + np.take(a, idx, axis=axis) * wk.reshape(shape)
    return out


def smooth_images(rng, V, H, W):
    """Smooth images that correlate between the views, (V, H, W, 3) uint8: one low-resolution noise field upsampled,
    shifted by a few pixels per view, plus a little per-view noise. Smoothness is what keeps the scores non-uniform."""
    low = rng.uniform(0, 1, (3, H // 8 + 4, W // 8 + 4))
    big = _cubic_axis(_cubic_axis(low, 1, H + 32), 2, W + 32)
    out = np.zeros((V, H, W, 3), np.uint8)
    for v in range(V):
        dy, dx = (int(s) for s in rng.integers(0, 12, 2))
        crop = big[:, 8 + dy: 8 + dy + H, 8 + dx: 8 + dx + W].transpose(1, 2, 0)
        out[v] = np.clip((crop + rng.uniform(-0.035, 0.035, crop.shape)) * 255.0, 0, 255).astype(np.uint8)
    return out


def _case(seed, H, W, wRc, wtc, intrinsics, depth_range, src_views):
    rng = np.random.default_rng(seed)
    V = len(wtc)
    case = dict(images=smooth_images(rng, V, H, W), wRc=np.stack(wRc), wtc=np.array(wtc, np.float64),
                intrinsics=np.array(intrinsics, np.float64), depth_range=np.array(depth_range, np.float64),
                src_views=np.array(src_views, np.int32))
    case["uniform"] = rng.uniform(0, 1, (pref.INIT_BINS, H // 8, W // 8)).astype(np.float32)
    return case


def cases():
    """{"c": case, "d": case} with the keys of a golden case's inputs: images, wRc, wtc, intrinsics, src_views,
    depth_range and view 0's uniform numbers (pref.batch_uniform seeds the other views')."""
    poses = [_rot(0, 0, 0), _rot(0.005, -0.015, 0.01), _rot(-0.01, 0.02, -0.005)]
    centres = [[0.0, 0.0, 0.0], [0.25, 0.02, 0.0], [-0.2, 0.05, 0.05]]
    return {
        "c": _case(SEEDS["c"], 16, 24, poses[:2], [[0.0, 0.0, 0.0], [0.2, 0.02, 0.0]],
                   [[26.0, 12.0, 8.0], [25.0, 11.5, 8.5]], [[2.5, 6.0], [2.2, 5.5]], [[1], [0]]),
        "d": _case(SEEDS["d"], 136, 152, poses, centres,
                   [[160.0, 76.0, 68.0], [155.0, 77.5, 67.0], [168.0, 74.5, 69.0]],
                   [[2.5, 6.0], [2.2, 5.5], [2.0, 5.0]], [[1, 2, -1], [-1, 0, 2], [7, 1, 0]]),
    }


def valid_sources(case, view):
    """The sources of a view the kernels use: its row's indices inside [0, n_views), in row order."""
    n = case["images"].shape[0]
    return [int(s) for s in case["src_views"][view] if 0 <= s < n]


def restatement(sd_np, case, view, dtype, uniform=None):
    """pref.run_case for `view` as the reference view with its valid sources and its uniform numbers (48, H/8, W/8);
    the default is the case's batch_uniform. Every output as a numpy array: iter0..4, depth, confidence, index."""
    uniform = pref.batch_uniform(case)[view] if uniform is None else uniform
    one = dict(case, src_views=[valid_sources(case, v) for v in range(case["images"].shape[0])])
    r = pref.run_case(sd_np, one, dtype, ref_view=view, uniform=uniform)
    out = {f"iter{i}": d.numpy() for i, d in enumerate(r["iter_depths"])}
    out.update(depth=r["depth"].numpy(), confidence=r["confidence"].numpy(), index=r["index"].numpy())
    return out
