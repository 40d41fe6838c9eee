"""The reference's track estimation restated in numpy / scipy, and seeded scenes for it.

Route restated: gtsfm/data_association/dsf_tracks_estimator.py:56-85 (one dsf.merge per correspondence row, dsf.sets(),
one candidate track per set, the set dropped when two of its keypoints share an image:
gtsfm/common/sfm_track.py:105-112). Connected components come from scipy.sparse.csgraph instead of gtsam's DSFMap, the
sets are the same. Output order is the project's canonical one: tracks by ascending smallest node id (i * kmax + k),
measurements by ascending node id inside a track.
"""
import json
import os
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tracks")
GOLDEN_CASES = ("three_images", "dummy_matches", "malformed_same_image", "nontransitive")


class RefTracks(NamedTuple):
    offsets: np.ndarray  # (n_tracks + 1,) int32
    image: np.ndarray  # (n_measurements,) int32
    keypoint: np.ndarray  # (n_measurements,) int32
    uv: Optional[np.ndarray]  # (n_measurements, 2) float32, None without kp_xy
    stats: np.ndarray  # (5,) int64: n_tracks, n_measurements, n_components, n_erroneous, n_bad_rows

    def track_lengths(self) -> np.ndarray:
        return np.diff(self.offsets)


def reference_tracks(pairs, offsets, v_corr, kp_count, kmax: int, valid=None, kp_xy=None) -> RefTracks:
    """Tracks of a CSR of correspondences (pair p owns rows offsets[p] .. offsets[p + 1] of v_corr)."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    offsets = np.asarray(offsets, np.int64)
    v_corr = np.asarray(v_corr).astype(np.int64).reshape(-1, 2)
    kp_count = np.asarray(kp_count, np.int64)
    n_img, P = len(kp_count), len(pairs)
    n_rows = int(offsets[P]) if P else 0
    pair_of_row = np.repeat(np.arange(P), np.diff(offsets[: P + 1]))
    rows = v_corr[int(offsets[0]) if P else 0: n_rows]
    use = np.ones(len(rows), bool) if valid is None else np.asarray(valid).astype(bool)[pair_of_row]
    i1, i2 = pairs[pair_of_row, 0], pairs[pair_of_row, 1]
    img_ok = (i1 >= 0) & (i1 < n_img) & (i2 >= 0) & (i2 < n_img)
    lim1 = np.minimum(kp_count[np.clip(i1, 0, max(n_img - 1, 0))], kmax) if n_img else np.zeros(len(rows), np.int64)
    lim2 = np.minimum(kp_count[np.clip(i2, 0, max(n_img - 1, 0))], kmax) if n_img else np.zeros(len(rows), np.int64)
    row_ok = img_ok & (rows[:, 0] >= 0) & (rows[:, 0] < lim1) & (rows[:, 1] >= 0) & (rows[:, 1] < lim2)
    n_bad_rows = int((use & ~row_ok).sum())
    sel = use & row_ok
    u = i1[sel] * kmax + rows[sel, 0]
    v = i2[sel] * kmax + rows[sel, 1]
    nodes = np.unique(np.concatenate([u, v]))  # touched nodes, ascending
    if len(nodes) == 0:
        uv = None if kp_xy is None else np.zeros((0, 2), np.float32)
        return RefTracks(np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), uv,
                         np.array([0, 0, 0, 0, n_bad_rows], np.int64))
    a, b = np.searchsorted(nodes, u), np.searchsorted(nodes, v)
    graph = coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(len(nodes), len(nodes)))
    n_components, label = connected_components(graph, directed=False)
    first = np.full(n_components, np.iinfo(np.int64).max, np.int64)  # smallest node of every component
    np.minimum.at(first, label, nodes)
    root = first[label]
    order = np.lexsort((nodes, root))  # by (smallest node of the component, node)
    s_nodes, s_root = nodes[order], root[order]
    s_img = s_nodes // kmax
    same = (s_root[1:] == s_root[:-1]) & (s_img[1:] == s_img[:-1])  # adjacent members in one image
    bad_roots = np.unique(s_root[1:][same])
    keep = ~np.isin(s_root, bad_roots)
    t_nodes, t_root = s_nodes[keep], s_root[keep]
    starts = np.flatnonzero(np.concatenate([[True], t_root[1:] != t_root[:-1]])) if len(t_nodes) else np.zeros(0, int)
    t_offsets = np.concatenate([starts, [len(t_nodes)]]).astype(np.int32)
    image = (t_nodes // kmax).astype(np.int32)
    keypoint = (t_nodes % kmax).astype(np.int32)
    uv = None
    if kp_xy is not None:
        uv = np.asarray(kp_xy, np.float32).reshape(n_img, kmax, 2)[image, keypoint]
    stats = np.array([len(starts), len(t_nodes), n_components, len(bad_roots), n_bad_rows], np.int64)
    return RefTracks(t_offsets, image, keypoint, uv, stats)


def csr_from_dict(matches_dict: Dict[Tuple[int, int], np.ndarray]) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(pairs, offsets, v_corr) of a dict (i1, i2) -> (K, 2) rows, in dict order."""
    pairs = np.array(list(matches_dict.keys()), np.int32).reshape(-1, 2)
    rows = [np.asarray(r, np.int32).reshape(-1, 2) for r in matches_dict.values()]
    offsets = np.zeros(len(rows) + 1, np.int32)
    np.cumsum([len(r) for r in rows], out=offsets[1:])
    v_corr = np.concatenate(rows) if rows else np.zeros((0, 2), np.int32)
    return pairs, offsets, v_corr


def pack_keypoints(coords: List[np.ndarray]) -> Tuple[np.ndarray, int, np.ndarray]:
    """(kp_count, kmax, kp_xy[n_img][kmax][2] float32) of per-image (K, 2) coordinate arrays."""
    kp_count = np.array([len(c) for c in coords], np.int32)
    kmax = max(int(kp_count.max()) if len(coords) else 0, 1)
    kp_xy = np.zeros((len(coords), kmax, 2), np.float32)
    for i, c in enumerate(coords):
        kp_xy[i, : len(c)] = c
    return kp_count, kmax, kp_xy


def reference_tracks_from_dict(matches_dict, coords: List[np.ndarray]) -> RefTracks:
    kp_count, kmax, kp_xy = pack_keypoints(coords)
    pairs, offsets, v_corr = csr_from_dict(matches_dict)
    return reference_tracks(pairs, offsets, v_corr, kp_count, kmax, None, kp_xy)


def load_golden(name: str):
    """(matches_dict, per-image coordinate arrays, the case's dict) of tests/golden/tracks/<name>.json."""
    with open(os.path.join(GOLDEN_DIR, name + ".json")) as f:
        case = json.load(f)
    coords = [np.array(c, np.float64).reshape(-1, 2) for c in case["keypoints"]]
    matches = {tuple(m["pair"]): np.array(m["rows"], np.int64).reshape(-1, 2) for m in case["matches"]}
    return matches, coords, case


class Scene(NamedTuple):
    pairs: np.ndarray  # (P, 2) int32
    offsets: np.ndarray  # (P + 1,) int32
    v_corr: np.ndarray  # (rows, 2) int32
    kp_count: np.ndarray  # (n_img,) int32
    kmax: int
    valid: Optional[np.ndarray]  # (P,) uint8 or None
    kp_xy: np.ndarray  # (n_img, kmax, 2) float32


def shuffle_rows(scene: Scene, seed: int) -> Scene:
    """The same set of rows with the pairs, and the rows inside every pair, in another order."""
    rng = np.random.default_rng(seed)
    P = len(scene.pairs)
    perm = rng.permutation(P)
    counts = np.diff(scene.offsets)[perm]
    offsets = np.zeros(P + 1, np.int32)
    np.cumsum(counts, out=offsets[1:])
    chunks = []
    for p in perm:
        rows = scene.v_corr[scene.offsets[p]: scene.offsets[p + 1]]
        chunks.append(rows[rng.permutation(len(rows))])
    v_corr = np.concatenate(chunks) if chunks else scene.v_corr
    valid = None if scene.valid is None else scene.valid[perm]
    return scene._replace(pairs=scene.pairs[perm], offsets=offsets, v_corr=v_corr, valid=valid)


def make_scene(n_img: int, kp_per_img: int, n_points: int, vis_prob: float, wrong_share: float = 0.0,
               masked_share: float = 0.0, shuffle: bool = False, seed: int = 0, match_prob: float = 1.0,
               vis_spread: float = 0.0) -> Scene:
    """Correspondences of n_points latent 3D points over all image pairs.

    Point j is seen by an image with probability vis_prob * (1 - vis_spread * u_j), u_j uniform in [0, 1) per point
    (vis_spread > 0 mixes long and short tracks); an image gives each point it sees its own keypoint slot (at most
    kp_per_img of them, the rest of the slots stay unmatched). A pair's rows are the points both images see, each
    kept with probability match_prob; a share wrong_share of all rows gets a random second keypoint instead (a wrong
    match); a share masked_share of the pairs is flagged valid = 0; shuffle reorders pairs and rows."""
    rng = np.random.default_rng(seed)
    p_point = vis_prob * (1.0 - vis_spread * rng.random(n_points))
    vis = rng.random((n_img, n_points)) < p_point[None, :]
    slot = np.full((n_img, n_points), -1, np.int64)
    for i in range(n_img):
        seen = np.flatnonzero(vis[i])
        if len(seen) > kp_per_img:
            vis[i, seen[kp_per_img:]] = False
            seen = seen[:kp_per_img]
        slot[i, seen] = rng.permutation(kp_per_img)[: len(seen)]
    pairs, counts, chunks = [], [], []
    for i in range(n_img - 1):
        common = vis[i][None, :] & vis[i + 1:]
        if match_prob < 1.0:
            common &= rng.random(common.shape) < match_prob
        dj, pt = np.nonzero(common)  # ordered by second image, then point
        j = i + 1 + dj
        chunks.append(np.stack([slot[i, pt], slot[j, pt]], axis=1))
        pairs.append(np.stack([np.full(n_img - 1 - i, i), np.arange(i + 1, n_img)], axis=1))
        counts.append(np.bincount(dj, minlength=n_img - 1 - i))
    pairs = np.concatenate(pairs).astype(np.int32) if pairs else np.zeros((0, 2), np.int32)
    counts = np.concatenate(counts) if counts else np.zeros(0, np.int64)
    v_corr = (np.concatenate(chunks) if chunks else np.zeros((0, 2), np.int64)).astype(np.int32)
    wrong = rng.random(len(v_corr)) < wrong_share
    v_corr[wrong, 1] = rng.integers(0, kp_per_img, int(wrong.sum()))
    offsets = np.zeros(len(pairs) + 1, np.int32)
    np.cumsum(counts, out=offsets[1:])
    valid = None
    if masked_share > 0:
        valid = (rng.random(len(pairs)) >= masked_share).astype(np.uint8)
    kp_count = np.full(n_img, kp_per_img, np.int32)
    kp_xy = rng.random((n_img, kp_per_img, 2), dtype=np.float32) * np.float32(1000.0)
    scene = Scene(pairs, offsets, v_corr, kp_count, kp_per_img, valid, kp_xy)
    return shuffle_rows(scene, seed + 1) if shuffle else scene


def scene_as_dict(scene: Scene) -> Dict[Tuple[int, int], np.ndarray]:
    """The valid pairs of a scene as a matches dict (pairs must be distinct)."""
    out = {}
    for p, (i1, i2) in enumerate(scene.pairs):
        if scene.valid is None or scene.valid[p]:
            out[(int(i1), int(i2))] = scene.v_corr[scene.offsets[p]: scene.offsets[p + 1]]
    return out
