"""Packed two-view batches whose indices are all non-trivial (test infrastructure for the two-view entry points:
gtsfm_ransac_E_batched, gtsfm_ransac_F_batched, gtsfm_ba2_batched and the Ransac plugin above them).

pack() lays pairs out the way the all-pairs engine does -- images shared between pairs, one calibration per image,
keypoint slots in an order unrelated to the putative order, kmax != mcap, decoys in every slot and row a correct
kernel never reads -- and returns, next to the ABI arrays, each pair's pixels in putative order. Expected values are
computed from those, never by gathering through the packed indices again.

The F-path edge inputs (putative counts around the LMedS / wave boundaries, degenerate pairs) live here too, so the
CPU companion and the GPU test look at the same arrays.
"""
import dataclasses
from typing import List, Tuple

import numpy as np

from tests import scenes

DECOY = (1e6, -1e6)  # finite, far outside any image: a slot or row read by mistake wrecks the estimate, not the GPU

# (f, u0, v0) per image: different enough that a mix-up is gross. Image 3 repeats image 0's calibration (control).
IMAGE_K = [(1000.0, 960.0, 540.0), (1400.0, 700.0, 500.0), (800.0, 1010.0, 610.0), (1000.0, 960.0, 540.0),
           (1200.0, 900.0, 560.0)]
# every image in more than one pair; 0, 1, 2, 3 and 4 each first in one pair and second in another; (2, 0), (4, 1),
# (4, 2) and (3, 1) have i1 > i2; (0, 3) has the same K on both sides
PAIR_IMAGES = [(0, 1), (1, 2), (2, 0), (0, 3), (3, 4), (4, 1), (4, 2), (3, 1)]
PAIR_SIZES = [(150, 70), (90, 60), (200, 120), (120, 50), (160, 80), (180, 90), (100, 100), (45, 20)]  # (n_in, n_out)
PAIR_IDS = [11, 3, 40, 7, 0, 129, 65, 1000]  # explicit sampler keys, neither sequential nor sorted
# with 0.5 px noise on both views a 0.75 px threshold cuts through the true correspondences' residuals, so scaling it
# by the wrong focal length (0.75 / 1000 instead of 0.75 / 1400) moves a visible share of them across it
THR_PX = 0.75
F_MAX_ITERS = 20000  # F path: far above what these pairs need, small enough that a garbage input ends quickly
SCENE_SEED = 77
LAYOUTS = ("wide", "tall")  # kmax > mcap / kmax < mcap


@dataclasses.dataclass
class Batch:
    kp: np.ndarray            # (n_img, kmax, 2) float32
    intr: np.ndarray          # (n_img, 3) float64 (f, u0, v0)
    pairs: np.ndarray         # (P, 2) int32
    match_idx: np.ndarray     # (P, mcap, 2) int32
    match_count: np.ndarray   # (P,) int32
    x1: List[np.ndarray]      # per pair (M, 2) float32 pixels of the first image, putative order
    x2: List[np.ndarray]      # ... of the second image
    K1: List[Tuple[float, float, float]]
    K2: List[Tuple[float, float, float]]
    n_slots: np.ndarray       # (n_img,) keypoint slots in use per image; slots at or past it hold DECOY

    @property
    def kmax(self) -> int:
        return self.kp.shape[1]

    @property
    def mcap(self) -> int:
        return self.match_idx.shape[1]

    def reversed(self) -> "Batch":
        """The same batch with the pairs in reverse order (images untouched)."""
        r = slice(None, None, -1)
        return dataclasses.replace(self, pairs=np.ascontiguousarray(self.pairs[r]),
                                   match_idx=np.ascontiguousarray(self.match_idx[r]),
                                   match_count=np.ascontiguousarray(self.match_count[r]), x1=self.x1[r], x2=self.x2[r],
                                   K1=self.K1[r], K2=self.K2[r])


def pack(pair_scenes, pair_images, image_K, rng, kmax_pad: int = 5, mcap_pad: int = 3) -> Batch:
    """pair_scenes[p] = (uv1, uv2): (M, 2) pixels of pair p in images pair_images[p] = (i1, i2); image_K[i] =
    (f, u0, v0). kmax = the fullest image + kmax_pad (>= 1: every image keeps a decoy slot), mcap = the largest pair +
    mcap_pad."""
    assert kmax_pad >= 1 and mcap_pad >= 0
    n_img, P = len(image_K), len(pair_scenes)
    counts = np.array([len(s[0]) for s in pair_scenes], np.int32)
    n_slots = np.zeros(n_img, np.int64)
    for (i1, i2), m in zip(pair_images, counts):
        assert i1 != i2
        n_slots[i1] += m
        n_slots[i2] += m
    kmax, mcap = int(n_slots.max()) + kmax_pad, int(counts.max()) + mcap_pad
    kp = np.empty((n_img, kmax, 2), np.float32)
    kp[:] = DECOY
    match_idx = np.zeros((P, mcap, 2), np.int32)
    fill = np.zeros(n_img, np.int64)
    x1s, x2s = [], []
    for p, ((uv1, uv2), (i1, i2)) in enumerate(zip(pair_scenes, pair_images)):
        m = int(counts[p])
        order = rng.permutation(m)  # putative order
        x1, x2 = np.asarray(uv1)[order].astype(np.float32), np.asarray(uv2)[order].astype(np.float32)
        for col, (img, x) in enumerate(((i1, x1), (i2, x2))):
            slot = fill[img] + rng.permutation(m)  # this pair's block of the image, permuted on its own
            kp[img, slot] = x
            match_idx[p, :m, col] = slot
            fill[img] += m
            # rows past the putatives: in range, pointing at decoy slots
            match_idx[p, m:, col] = rng.integers(n_slots[img], kmax, size=mcap - m)
        x1s.append(x1)
        x2s.append(x2)
    assert np.array_equal(fill, n_slots)
    return Batch(kp=kp, intr=np.array(image_K, np.float64), pairs=np.array(pair_images, np.int32),
                 match_idx=match_idx, match_count=counts, x1=x1s, x2=x2s, K1=[image_K[a] for a, _ in pair_images],
                 K2=[image_K[b] for _, b in pair_images], n_slots=n_slots)


def standard_scenes():
    """The eight scenes of the standard batch: (uv1, uv2, R, t) per pair, each view projected with its image's K."""
    rng = np.random.default_rng(SCENE_SEED)
    out = []
    for (i1, i2), (n_in, n_out) in zip(PAIR_IMAGES, PAIR_SIZES):
        uv1, uv2, R, t, _ = scenes.random_two_view_k(rng, n_in, n_out, IMAGE_K[i1], IMAGE_K[i2])
        out.append((uv1, uv2, R, t))
    return out


def standard_batch(layout: str):
    """(Batch, ground truth [(R, t)]) of the standard scenes; "wide" has kmax > mcap, "tall" kmax < mcap (the putative
    arrays padded past the fullest image). The two layouts permute slots and rows differently."""
    sc = standard_scenes()
    rng = np.random.default_rng({"wide": 101, "tall": 202}[layout])
    kmax_full = max(sum(len(s[0]) for s, pi in zip(sc, PAIR_IMAGES) if i in pi) for i in range(len(IMAGE_K)))
    m_full = max(len(s[0]) for s in sc)
    kw = dict(kmax_pad=5, mcap_pad=3) if layout == "wide" else dict(kmax_pad=2, mcap_pad=kmax_full - m_full + 39)
    b = pack([(s[0], s[1]) for s in sc], PAIR_IMAGES, IMAGE_K, rng, **kw)
    assert (b.kmax > b.mcap) if layout == "wide" else (b.kmax < b.mcap)
    return b, [(s[2], s[3]) for s in sc]


def normalise(x, K):
    """(float32 px as float64 - (u0, v0)) / f: utils/features.py normalize_coordinates for a Cal3Bundler without
    distortion."""
    return (np.asarray(x, np.float32).astype(np.float64) - np.array(K[1:])) / K[0]


def k_matrix(K):
    f, u0, v0 = K
    return np.array([[f, 0.0, u0], [0.0, f, v0], [0.0, 0.0, 1.0]])


# ---- F-path edges ----------------------------------------------------------------------------------------------
F_EDGE_COUNTS = (7, 8, 14, 15, 16, 63, 64, 65, 128, 129)
F_EDGE_K = (1000.0, 960.0, 540.0)


def f_edge_pairs():
    """One pair per putative count in F_EDGE_COUNTS, 0.5 px noise: two gross outliers in the LMedS range
    (8 <= M < 15), ~30 % outliers from M = 15 on, none for the too-small M = 7. Returns [(x1, x2)] float32."""
    rng = np.random.default_rng(404)
    out = []
    for M in F_EDGE_COUNTS:
        n_out = 0 if M < 8 else 2 if M < 15 else int(round(0.3 * M))
        a, b, _, _, _ = scenes.random_two_view_k(rng, M - n_out, n_out, F_EDGE_K, F_EDGE_K)
        assert len(a) == M
        out.append((a.astype(np.float32), b.astype(np.float32)))
    return out


def f_max_iters_pair():
    """M = 200 with 35 % outliers: needs more than one batch of 64 hypotheses, so a max_iters cap bites."""
    rng = np.random.default_rng(405)
    a, b, _, _, _ = scenes.random_two_view_k(rng, 130, 70, F_EDGE_K, F_EDGE_K)
    assert len(a) == 200
    return a.astype(np.float32), b.astype(np.float32)


def f_degenerate_pairs():
    """30 putatives each: all on one line in image 1 (exactly: a constant y), and all at one point in both images.
    Every 7-sample holds a collinear triple, so no hypothesis is ever formed."""
    rng = np.random.default_rng(406)
    line1 = np.stack([rng.uniform(100, 1800, 30), np.full(30, 300.0)], 1)
    line2 = np.stack([rng.uniform(0, 1920, 30), rng.uniform(0, 1080, 30)], 1)
    point1, point2 = np.tile([[640.25, 360.5]], (30, 1)), np.tile([[700.0, 410.75]], (30, 1))
    return [(line1.astype(np.float32), line2.astype(np.float32)),
            (point1.astype(np.float32), point2.astype(np.float32))]


def f_ordinary_pair(seed: int):
    rng = np.random.default_rng(seed)
    a, b, _, _, _ = scenes.random_two_view_k(rng, 80, 30, F_EDGE_K, F_EDGE_K)
    return a.astype(np.float32), b.astype(np.float32)


def pack_private(pairs_xy, K=F_EDGE_K, mcap_pad: int = 5):
    """Pairs with private images (2p, 2p + 1) and identity indices, decoys past each pair's count: the plain layout for
    tests that are about the estimator's edges, not the gather. Returns kp, intr, pairs, match_idx, match_count."""
    P = len(pairs_xy)
    counts = np.array([len(a) for a, _ in pairs_xy], np.int32)
    kmax = int(counts.max()) + 1
    mcap = int(counts.max()) + mcap_pad
    kp = np.empty((2 * P, kmax, 2), np.float32)
    kp[:] = DECOY
    mi = np.full((P, mcap, 2), kmax - 1, np.int32)
    for p, (a, b) in enumerate(pairs_xy):
        kp[2 * p, : len(a)], kp[2 * p + 1, : len(b)] = a, b
        mi[p, : len(a)] = np.arange(len(a))[:, None]
    intr = np.tile(np.array(K, np.float64), (2 * P, 1))
    return kp, intr, np.arange(2 * P, dtype=np.int32).reshape(P, 2), mi, counts
