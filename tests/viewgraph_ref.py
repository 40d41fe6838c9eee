"""numpy / scipy restatement of the reference's cycle-consistent rotation filter, and seeded view-graph scenes.

Not a test: tests/test_viewgraph.py pins it to the reference's own known answers, tests/test_viewgraph_gpu.py compares
the HIP kernel against it. The route is the reference's (cycle_consistent_rotation_estimator.py:78-152):
  triplets by adjacency-set intersection (graph.py:100-135), M = R(i0,i2)^T R(i1,i2) R(i0,i1) for i0 < i1 < i2
  (geometry_comparisons.py:355-370), angle = rad2deg(|Rotation.from_matrix(M).as_rotvec()|) (:266-288, scipy as the
  reference uses it), np.amin / np.median per edge, strict < against the threshold.
The angle is vectorised over all triplets, so a 300-image complete graph (4.4 M triplets) takes seconds.
"""
from collections import defaultdict
from typing import Dict, Iterable, List, NamedTuple, Optional, Set, Tuple

import numpy as np
from scipy.spatial.transform import Rotation

MIN_EDGE_ERROR = "MIN_EDGE_ERROR"
MEDIAN_EDGE_ERROR = "MEDIAN_EDGE_ERROR"
ERROR_THRESHOLD = 7.0


def extract_triplets_sets(edges: Iterable[Tuple[int, int]]) -> List[Tuple[int, int, int]]:
    """Sorted 3-tuples of images whose three edges are all present: for every edge, the intersection of its two
    ends' adjacency sets (graph.py:100-135)."""
    adj: Dict[int, Set[int]] = defaultdict(set)
    edges = [tuple(int(v) for v in e) for e in edges]
    for a, b in edges:
        adj[a].add(b)
        adj[b].add(a)
    out = set()
    for a, b in edges:
        for c in adj[a] & adj[b]:
            out.add(tuple(sorted((a, b, c))))
    return sorted(out)


def extract_triplets(pairs: np.ndarray) -> np.ndarray:
    """The same triplets as extract_triplets_sets, as a (T, 3) int64 array in lexicographic order, from a dense
    adjacency matrix (tests/test_viewgraph.py checks the two against each other)."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if len(pairs) == 0:
        return np.zeros((0, 3), np.int64)
    n = int(pairs.max()) + 1
    adj = np.zeros((n, n), bool)
    adj[pairs[:, 0], pairs[:, 1]] = True
    adj[pairs[:, 1], pairs[:, 0]] = True
    np.fill_diagonal(adj, False)
    out = []
    for i0 in range(n):
        nb = np.flatnonzero(adj[i0, i0 + 1:]) + i0 + 1
        if len(nb) < 2:
            continue
        j, k = np.nonzero(np.triu(adj[np.ix_(nb, nb)], 1))
        out.append(np.stack([np.full(len(j), i0, np.int64), nb[j], nb[k]], axis=1))
    return np.concatenate(out) if out else np.zeros((0, 3), np.int64)


def rotation_angle_deg(M: np.ndarray) -> np.ndarray:
    """(T, 3, 3) -> (T,) rotation angles in degrees by the scipy route; NaN where M is not finite."""
    M = np.asarray(M, dtype=np.float64).reshape(-1, 3, 3)
    out = np.full(len(M), np.nan)
    ok = np.isfinite(M).all(axis=(1, 2))
    if ok.any():
        out[ok] = np.rad2deg(np.linalg.norm(Rotation.from_matrix(M[ok]).as_rotvec(), axis=1))
    return out


def cyclic_rotation_error_deg(i1Ri0: np.ndarray, i2Ri1: np.ndarray, i2Ri0: np.ndarray) -> np.ndarray:
    """compute_cyclic_rotation_error (geometry_comparisons.py:355-370) on (..., 3, 3) stacks."""
    M = np.swapaxes(np.asarray(i2Ri0), -1, -2) @ np.asarray(i2Ri1) @ np.asarray(i1Ri0)
    return rotation_angle_deg(M)


class RefResult(NamedTuple):
    keep: np.ndarray  # (P,) bool
    agg_error_deg: np.ndarray  # (P,) float64, NaN where the pair is invalid or in no triplet
    n_triplets: np.ndarray  # (P,) int32
    total_triplets: int


class RefCycles:
    """The cycle errors of a view graph, grouped per edge (the reference's per_edge_errors): computed once, aggregated
    by either criterion. pairs (P, 2) with i1 < i2 in any order, R (P, 3, 3) i2Ri1, valid (P,) or None (the graph is
    then the valid subset alone)."""

    def __init__(self, pairs: np.ndarray, R: np.ndarray, valid: Optional[np.ndarray] = None, chunk: int = 1 << 20):
        pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        R = np.asarray(R, dtype=np.float64).reshape(-1, 3, 3)
        self.n_pairs = P = len(pairs)
        self.total_triplets = 0
        self.per_edge_errors: Dict[int, np.ndarray] = {}  # pair index -> cycle errors of its triplets
        sel = np.arange(P) if valid is None else np.flatnonzero(np.asarray(valid).reshape(P) != 0)
        sel = sel[pairs[sel, 0] < pairs[sel, 1]]
        trip = extract_triplets(pairs[sel])
        if len(trip) == 0:
            return
        n = int(pairs[sel].max()) + 1
        idx = np.full((n, n), -1, np.int64)
        idx[pairs[sel, 0], pairs[sel, 1]] = sel
        e01, e12, e02 = idx[trip[:, 0], trip[:, 1]], idx[trip[:, 1], trip[:, 2]], idx[trip[:, 0], trip[:, 2]]
        err = np.empty(len(trip))
        for s in range(0, len(trip), chunk):
            t = slice(s, s + chunk)
            err[t] = cyclic_rotation_error_deg(R[e01[t]], R[e12[t]], R[e02[t]])
        edge_of = np.concatenate([e01, e12, e02])
        order = np.argsort(edge_of, kind="stable")
        err3 = np.concatenate([err, err, err])[order]
        ids, start, counts = np.unique(edge_of[order], return_index=True, return_counts=True)
        self.per_edge_errors = {int(e): err3[s: s + c] for e, s, c in zip(ids, start, counts)}
        self.total_triplets = len(trip)

    def filter(self, criterion: str = MEDIAN_EDGE_ERROR, threshold: float = ERROR_THRESHOLD) -> RefResult:
        agg = np.full(self.n_pairs, np.nan)
        n_trip = np.zeros(self.n_pairs, np.int32)
        fn = {MIN_EDGE_ERROR: np.amin, MEDIAN_EDGE_ERROR: np.median}[criterion]
        with np.errstate(invalid="ignore"):
            for e, errors in self.per_edge_errors.items():
                agg[e] = fn(errors)
                n_trip[e] = len(errors)
            keep = agg < threshold  # False for NaN: an edge in no triplet, or with a NaN cycle error, is dropped
        return RefResult(keep, agg, n_trip, self.total_triplets)


def reference_filter(pairs: np.ndarray, R: np.ndarray, valid: Optional[np.ndarray] = None,
                     criterion: str = MEDIAN_EDGE_ERROR, threshold: float = ERROR_THRESHOLD) -> RefResult:
    """The reference's run() on arrays; results in input order."""
    return RefCycles(pairs, R, valid).filter(criterion, threshold)


def reference_filter_edges(pairs: np.ndarray, R: np.ndarray, edge_ids: np.ndarray, criterion: str = MEDIAN_EDGE_ERROR,
                           threshold: float = ERROR_THRESHOLD, chunk: int = 256) -> RefResult:
    """reference_filter's rows for the chosen edges only, for graphs whose whole triplet list is too long to hold
    (1000 images: 166 M): the common neighbours of each chosen edge from a dense adjacency matrix, the same cycle
    error, the same aggregation. Every pair is an edge (i1 < i2, no mask). total_triplets is not computed (-1)."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    R = np.asarray(R, dtype=np.float64).reshape(-1, 3, 3)
    edge_ids = np.asarray(edge_ids, dtype=np.int64)
    n = int(pairs.max()) + 1
    idx = np.full((n, n), -1, np.int64)
    idx[pairs[:, 0], pairs[:, 1]] = np.arange(len(pairs))
    idx[pairs[:, 1], pairs[:, 0]] = np.arange(len(pairs))
    adj = idx >= 0
    fn = {MIN_EDGE_ERROR: np.amin, MEDIAN_EDGE_ERROR: np.median}[criterion]
    agg = np.full(len(edge_ids), np.nan)
    n_trip = np.zeros(len(edge_ids), np.int32)
    for s in range(0, len(edge_ids), chunk):
        ids = edge_ids[s: s + chunk]
        k, c = np.nonzero(adj[pairs[ids, 0]] & adj[pairs[ids, 1]])
        tri = np.sort(np.stack([pairs[ids[k], 0], pairs[ids[k], 1], c], axis=1), axis=1)
        err = cyclic_rotation_error_deg(R[idx[tri[:, 0], tri[:, 1]]], R[idx[tri[:, 1], tri[:, 2]]],
                                        R[idx[tri[:, 0], tri[:, 2]]])
        bounds = np.searchsorted(k, np.arange(len(ids) + 1))
        with np.errstate(invalid="ignore"):
            for j in range(len(ids)):
                if bounds[j + 1] > bounds[j]:
                    agg[s + j] = fn(err[bounds[j]: bounds[j + 1]])
                    n_trip[s + j] = bounds[j + 1] - bounds[j]
    with np.errstate(invalid="ignore"):
        return RefResult(agg < threshold, agg, n_trip, -1)


def threshold_margin(ref: RefResult, threshold: float = ERROR_THRESHOLD) -> float:
    """Distance in degrees from the threshold to the closest finite aggregate."""
    d = np.abs(ref.agg_error_deg[np.isfinite(ref.agg_error_deg)] - threshold)
    return float(d.min()) if len(d) else np.inf


def _small_rotations(rng: np.random.Generator, n: int, sigma_deg: float) -> np.ndarray:
    """n rotations about random axes whose angle is |N(0, sigma_deg)|."""
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    angle = np.deg2rad(sigma_deg) * np.abs(rng.normal(size=(n, 1)))
    return Rotation.from_rotvec(axis * angle).as_matrix()


def make_scene(n_img: int, seed: int, edge_prob: float = 1.0, noise_deg: float = 1.0, outlier_share: float = 0.1,
               outlier_deg: float = 25.0) -> Tuple[np.ndarray, np.ndarray]:
    """A seeded view graph: random global rotations wRi, every pair i1 < i2 kept with probability edge_prob, relative
    rotations i2Ri1 = noise * i2Rw * wRi1 with about noise_deg of noise, a share of them gross outliers (about
    outlier_deg). Returns (pairs (P, 2) int32 sorted by (i1, i2), R (P, 3, 3) float64)."""
    rng = np.random.default_rng(seed)
    wRi = Rotation.random(n_img, random_state=np.random.RandomState(seed)).as_matrix()
    i1, i2 = np.triu_indices(n_img, 1)
    sel = rng.random(len(i1)) < edge_prob
    i1, i2 = i1[sel], i2[sel]
    P = len(i1)
    sigma = np.where(rng.random(P) < outlier_share, outlier_deg, noise_deg)
    noise = np.empty((P, 3, 3))
    for s in np.unique(sigma):
        m = sigma == s
        noise[m] = _small_rotations(rng, int(m.sum()), float(s))
    R = noise @ np.swapaxes(wRi[i2], -1, -2) @ wRi[i1]
    return np.stack([i1, i2], axis=1).astype(np.int32), np.ascontiguousarray(R)


def ry(deg: float) -> np.ndarray:
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


# The reference's own scene (tests/view_graph_estimator/test_cycle_consistent_rotation_estimator.py): five cameras in
# a line with identity rotations, two triplets sharing image 2, the measurement of (2, 4) off by 15 degrees about y.
REFERENCE_SCENE_EDGES = [(0, 1), (1, 2), (0, 2), (2, 3), (3, 4), (2, 4)]
REFERENCE_SCENE_EXPECTED = {(0, 1), (1, 2), (0, 2)}


def reference_scene_rotations() -> Dict[Tuple[int, int], np.ndarray]:
    return {e: (ry(15.0) if e == (2, 4) else np.eye(3)) for e in REFERENCE_SCENE_EDGES}
