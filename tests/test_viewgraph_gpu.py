"""gtsfm_viewgraph_cycle_filter on the MI355X against tests/viewgraph_ref.py (the reference route in numpy / scipy).

Every comparison, for both criteria: n_triplets per edge and the total exactly; agg_error_deg within 1e-9 degrees
absolute (the kernel's atan2 formula and scipy's route differ by about 1e-13 on the CPU; the margin covers FMA
contraction and the device's atan2 / sqrt on angles up to 180 degrees); keep exactly, after asserting that the
restatement's closest aggregate is more than 1e-6 degrees from the threshold, so the tolerance cannot flip a decision
(a condition on the seeded inputs, not a skipped share).

The kernel has no per-pass capacity: its LDS is sized for n_img - 2 errors per edge, the most an edge can have, up to
the documented ceiling of 8192 images. It takes one of two paths by n_img: one wave per edge up to 512 images, four
waves above; `threshold500` runs one graph on both sides of that switch, and the complete graphs run through the
four-wave kernel as well (n_img = 513), so that all its waves hold errors.
"""
import functools

import numpy as np
import pytest
import torch

import viewgraph_ref as ref

pytestmark = pytest.mark.gpu

AGG_TOL_DEG = 1e-9
MARGIN_DEG = 1e-6
CRITERIA = (ref.MIN_EDGE_ERROR, ref.MEDIAN_EDGE_ERROR)


def _code(criterion):
    from gtsfm_amd import native

    return {ref.MIN_EDGE_ERROR: native.GTSFM_VG_MIN_EDGE_ERROR, ref.MEDIAN_EDGE_ERROR: native.GTSFM_VG_MEDIAN_EDGE_ERROR}[
        criterion]


def _gpu(pairs, R, valid, criterion, n_img=None, threshold=ref.ERROR_THRESHOLD):
    from gtsfm_amd import device

    dev = torch.device("cuda:0")
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    n_img = int(pairs.max()) + 1 if n_img is None else n_img
    v = None if valid is None else torch.from_numpy(np.asarray(valid, np.uint8)).to(dev)
    keep, agg, n_trip, total = device.viewgraph_cycle_filter(
        torch.from_numpy(pairs).to(dev), torch.from_numpy(np.ascontiguousarray(R, np.float64)).to(dev), v, n_img,
        _code(criterion), threshold)
    return keep.cpu().numpy().astype(bool), agg.cpu().numpy(), n_trip.cpu().numpy(), int(total.cpu()[0])


def _compare(got, want, label):
    keep, agg, n_trip, total = got
    assert ref.threshold_margin(want) > MARGIN_DEG, f"{label}: pick another seed, an aggregate sits on the threshold"
    np.testing.assert_array_equal(n_trip, want.n_triplets, err_msg=label)
    assert total == want.total_triplets, label
    np.testing.assert_array_equal(np.isnan(agg), np.isnan(want.agg_error_deg), err_msg=label)
    fin = np.isfinite(want.agg_error_deg)
    diff = float(np.abs(agg[fin] - want.agg_error_deg[fin]).max()) if fin.any() else 0.0
    print(f"{label}: {len(n_trip)} edges, {total} triplets, max |agg - ref| = {diff:.3e} deg, "
          f"threshold margin {ref.threshold_margin(want):.3e} deg")
    assert diff <= AGG_TOL_DEG, label
    np.testing.assert_array_equal(keep, want.keep, err_msg=label)


def _drop_image(pairs, R, image):
    m = (pairs != image).all(axis=1)
    return pairs[m], R[m]


@functools.lru_cache(maxsize=None)
def _scene(name):
    """(pairs, R, RefCycles) of a named scene: generated and evaluated by the restatement once, shared by the tests."""
    if name == "tri3":
        pairs, R = ref.make_scene(3, seed=1)
    elif name == "four_minus_one":  # triplets (0, 1, 2) and (0, 1, 3): edge (0, 1) is in two, (2, 3) is missing
        pairs, R = ref.make_scene(4, seed=2)
        pairs, R = pairs[:-1], R[:-1]
    elif name in ("p70_64", "p70_65", "p70_129"):  # across the 32-bit words of the adjacency rows
        pairs, R = ref.make_scene(int(name.split("_")[1]), seed=4, edge_prob=0.7)
    elif name == "sparse40":
        pairs, R = ref.make_scene(40, seed=5, edge_prob=0.12)
    elif name == "complete130":  # 128 triplets per edge: an even count
        pairs, R = ref.make_scene(130, seed=6, outlier_share=0.15)
    elif name == "complete130_minus_image":  # 127 per edge: an odd count
        pairs, R = _drop_image(*ref.make_scene(130, seed=6, outlier_share=0.15), image=77)
    elif name == "complete300":  # 298 per edge: more than one value per lane, more than 256
        pairs, R = ref.make_scene(300, seed=7)
    elif name == "threshold500":  # about 60 common neighbours per edge
        pairs, R = ref.make_scene(500, seed=8, edge_prob=0.35)
    else:
        raise KeyError(name)
    return pairs, R, ref.RefCycles(pairs, R)


@pytest.mark.parametrize("criterion", CRITERIA)
@pytest.mark.parametrize("name", ["tri3", "four_minus_one", "p70_64", "p70_65", "p70_129", "complete130",
                                  "complete130_minus_image", "complete300"])
def test_matches_restatement(name, criterion):
    pairs, R, cycles = _scene(name)
    want = cycles.filter(criterion)
    if name == "tri3":
        assert want.total_triplets == 1 and want.n_triplets.tolist() == [1, 1, 1]
    if name == "four_minus_one":
        assert want.total_triplets == 2 and sorted(want.n_triplets.tolist()) == [1, 1, 1, 1, 2]
    if name.startswith("complete"):
        n = {"complete130": 128, "complete130_minus_image": 127, "complete300": 298}[name]
        assert (want.n_triplets == n).all()
        assert 0 < want.keep.sum() < len(pairs)  # the outliers make the filter decide both ways
    _compare(_gpu(pairs, R, None, criterion), want, f"{name}/{criterion}")


@pytest.mark.parametrize("criterion", CRITERIA)
def test_sparse_graph_medians_of_one_and_two(criterion):
    """Edge probability 0.12: many edges are in no triplet (dropped, NaN aggregate), some in exactly one or two."""
    pairs, R, cycles = _scene("sparse40")
    want = cycles.filter(criterion)
    counts = want.n_triplets
    assert (counts == 0).sum() >= 5 and (counts == 1).sum() >= 3 and (counts == 2).sum() >= 1
    got = _gpu(pairs, R, None, criterion)
    _compare(got, want, f"sparse40/{criterion}")
    assert np.isnan(got[1][counts == 0]).all() and not got[0][counts == 0].any()


@pytest.mark.parametrize("criterion", CRITERIA)
@pytest.mark.parametrize("n_img", [512, 513])
def test_both_sides_of_the_wave_count_switch(n_img, criterion):
    """500 images given as n_img = 512 (one wave per edge) and 513 (four waves): the images past 499 are in no edge."""
    pairs, R, cycles = _scene("threshold500")
    _compare(_gpu(pairs, R, None, criterion, n_img=n_img), cycles.filter(criterion), f"threshold500@{n_img}/{criterion}")


@pytest.mark.parametrize("criterion", CRITERIA)
@pytest.mark.parametrize("name", ["complete130", "complete130_minus_image", "complete300"])
def test_four_wave_kernel_on_full_workgroups(name, criterion):
    """The complete graphs again under n_img = 513, which selects the four-wave kernel that serves every graph above
    512 images: 128 (even), 127 (odd) and 298 errors per edge, so waves 1 to 3 evaluate errors, add to the select's
    histogram and feed the cross-wave min / sum, and at 298 the select's loop takes a second trip."""
    pairs, R, cycles = _scene(name)
    _compare(_gpu(pairs, R, None, criterion, n_img=513), cycles.filter(criterion), f"{name}@513/{criterion}")


@pytest.mark.parametrize("criterion", CRITERIA)
def test_neighbours_spread_over_all_four_waves(criterion):
    """129 images renumbered 3, 53, 103, ... under n_img = 6500: the adjacency rows are 204 words long, so the common
    neighbours of an edge are found and compacted by all four waves of its workgroup."""
    pairs, R, cycles = _scene("p70_129")
    _compare(_gpu(pairs * 50 + 3, R, None, criterion, n_img=6500), cycles.filter(criterion), f"spread/{criterion}")


@pytest.mark.parametrize("criterion", CRITERIA)
def test_valid_mask_removes_adjacency(criterion):
    """An edge with valid = 0 closes no triplet: the result equals the restatement run on the valid subset alone."""
    pairs, R, _ = _scene("p70_65")
    valid = np.random.default_rng(0).random(len(pairs)) < 0.8
    want = ref.RefCycles(pairs, R, valid).filter(criterion)
    sub = ref.reference_filter(pairs[valid], R[valid], None, criterion)
    np.testing.assert_array_equal(want.agg_error_deg[valid], sub.agg_error_deg)
    got = _gpu(pairs, R, valid, criterion)
    _compare(got, want, f"valid/{criterion}")
    assert np.isnan(got[1][~valid]).all() and not got[0][~valid].any() and not got[2][~valid].any()


@pytest.mark.parametrize("criterion", CRITERIA)
def test_index_gaps_and_shuffled_order(criterion):
    """Image indices 5, 8, 11, ... (images that appear in no edge in between and past the end) with the edges in a
    shuffled order: results come back in input order."""
    pairs, R, cycles = _scene("p70_64")
    want = cycles.filter(criterion)
    perm = np.random.default_rng(1).permutation(len(pairs))
    gapped = (pairs * 3 + 5)[perm]
    got = _gpu(gapped, R[perm], None, criterion, n_img=int(gapped.max()) + 7)
    _compare(got, ref.RefResult(want.keep[perm], want.agg_error_deg[perm], want.n_triplets[perm], want.total_triplets),
             f"gaps+shuffle/{criterion}")


@pytest.mark.parametrize("criterion", CRITERIA)
def test_nan_rotation_drops_every_edge_it_touches(criterion):
    pairs, R, cycles = _scene("p70_65")
    clean = cycles.filter(criterion)
    bad = int(np.argmax(clean.n_triplets))
    Rn = R.copy()
    Rn[bad, 1, 2] = np.nan
    want = ref.reference_filter(pairs, Rn, None, criterion)
    touched = np.isnan(want.agg_error_deg) & ~np.isnan(clean.agg_error_deg)
    assert touched.sum() == 2 * clean.n_triplets[bad] + 1
    np.testing.assert_array_equal(want.agg_error_deg[~touched], clean.agg_error_deg[~touched])
    got = _gpu(pairs, Rn, None, criterion)
    _compare(got, want, f"nan/{criterion}")
    assert not got[0][touched].any()
    clean_gpu = _gpu(pairs, R, None, criterion)
    np.testing.assert_array_equal(got[1][~touched], clean_gpu[1][~touched])  # untouched edges: bit for bit


def test_zero_edges():
    from gtsfm_amd.view_graph_estimator.cycle_consistent_rotation_estimator import (
        CycleConsistentRotationViewGraphEstimator)

    keep, agg, n_trip, total = _gpu(np.zeros((0, 2), np.int32), np.zeros((0, 3, 3)), None, ref.MEDIAN_EDGE_ERROR, n_img=7)
    assert keep.shape == agg.shape == n_trip.shape == (0,) and total == 0
    est = CycleConsistentRotationViewGraphEstimator("MIN_EDGE_ERROR")
    assert [len(x) for x in est.run_arrays(np.zeros((0, 2), np.int64), np.zeros((0, 3, 3)))] == [0, 0, 0]
    assert est.run({}, {}, [], {}, [], {}) == set()


def test_argument_errors_with_device_buffers():
    """An unknown criterion and a short workspace return GTSFM_ERR_ARG and leave the outputs alone."""
    from gtsfm_amd import native

    lib = native.lib()
    dev = torch.device("cuda:0")
    pairs, R, _ = _scene("tri3")
    e = torch.from_numpy(pairs).to(dev)
    r = torch.from_numpy(R).to(dev)
    need = lib.gtsfm_viewgraph_workspace_bytes(3, 3)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    agg = torch.full((3,), -1.0, dtype=torch.float64, device=dev)
    n_trip = torch.full((3,), -1, dtype=torch.int32, device=dev)
    keep = torch.full((3,), 9, dtype=torch.uint8, device=dev)

    def call(criterion, ws_bytes):
        return lib.gtsfm_viewgraph_cycle_filter(e.data_ptr(), r.data_ptr(), None, 3, 3, criterion, 7.0, ws.data_ptr(),
                                                ws_bytes, agg.data_ptr(), n_trip.data_ptr(), keep.data_ptr(), None,
                                                native.stream_handle())

    assert call(2, need) == native.GTSFM_ERR_ARG
    assert call(native.GTSFM_VG_MEDIAN_EDGE_ERROR, need - 1) == native.GTSFM_ERR_ARG
    torch.cuda.synchronize()
    assert (agg == -1).all() and (n_trip == -1).all() and (keep == 9).all()
    assert call(native.GTSFM_VG_MEDIAN_EDGE_ERROR, need) == native.GTSFM_OK  # total_triplets NULL is allowed
    torch.cuda.synchronize()
    assert n_trip.tolist() == [1, 1, 1] and keep.tolist() == [1, 1, 1]


@pytest.mark.parametrize("criterion", CRITERIA)
def test_two_launches_are_bit_identical(criterion):
    pairs, R, _ = _scene("complete130")
    a = _gpu(pairs, R, None, criterion)
    b = _gpu(pairs, R, None, criterion)
    assert a[1].tobytes() == b[1].tobytes() and a[0].tobytes() == b[0].tobytes()


def test_run_arrays_device_tensors_equal_numpy_path():
    from gtsfm_amd.view_graph_estimator.cycle_consistent_rotation_estimator import (
        CycleConsistentRotationViewGraphEstimator, EdgeErrorAggregationCriterion)

    pairs, R, cycles = _scene("p70_129")
    valid = np.random.default_rng(2).random(len(pairs)) < 0.9
    est = CycleConsistentRotationViewGraphEstimator(EdgeErrorAggregationCriterion.MEDIAN_EDGE_ERROR)
    host = est.run_arrays(pairs.astype(np.int64), R, valid)
    assert all(isinstance(x, np.ndarray) for x in host)
    assert host[0].dtype == bool and host[1].dtype == np.float64 and host[2].dtype == np.int32
    dev = torch.device("cuda:0")
    out = est.run_arrays(torch.from_numpy(pairs).to(dev), torch.from_numpy(R).to(dev), torch.from_numpy(valid).to(dev),
                         num_images=129)
    assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in out) and out[0].dtype == torch.bool
    for h, d in zip(host, out):
        assert h.tobytes() == d.cpu().numpy().tobytes()
    cpu = est.run_arrays(torch.from_numpy(pairs), torch.from_numpy(R), torch.from_numpy(valid))
    assert all(isinstance(x, torch.Tensor) and not x.is_cuda for x in cpu)  # a tensor's results live where it does
    for h, c in zip(host, cpu):
        assert h.tobytes() == c.numpy().tobytes()
    want = ref.RefCycles(pairs, R, valid).filter(ref.MEDIAN_EDGE_ERROR)
    np.testing.assert_array_equal(host[0], want.keep)
    np.testing.assert_array_equal(host[2], want.n_triplets)


class _Rot:
    def __init__(self, R):
        self._R = R

    def matrix(self):
        return self._R


def test_reference_scene_through_run_and_estimate():
    """The reference's 5-image scene with dict inputs (Rot3-like values): MEDIAN keeps {(0,1), (1,2), (0,2)}; MIN too,
    every edge being in one triplet; estimate() returns four dicts keyed by exactly run()'s set."""
    from gtsfm_amd.view_graph_estimator.cycle_consistent_rotation_estimator import (
        CycleConsistentRotationViewGraphEstimator, EdgeErrorAggregationCriterion)

    rot = {e: _Rot(m) for e, m in ref.reference_scene_rotations().items()}
    i2Ui1 = {e: np.array([1.0, 0.0, 0.0]) for e in rot}
    corr = {e: np.zeros((0, 2), np.uint32) for e in rot}
    reports = {e: object() for e in rot}
    for crit in EdgeErrorAggregationCriterion:
        est = CycleConsistentRotationViewGraphEstimator(crit)
        edges = est.run(rot, i2Ui1, [None] * 5, corr, [None] * 5, reports)
        assert edges == ref.REFERENCE_SCENE_EXPECTED
        rot_in = dict(rot)
        rot_in[(1, 3)] = None  # dropped before run(): it closes no triplet
        rot_in[(4, 0)] = _Rot(np.eye(3))
        out = est.estimate(rot_in, {**i2Ui1, (1, 3): None, (4, 0): i2Ui1[(0, 1)]}, [None] * 5,
                           {**corr, (1, 3): None, (4, 0): None}, [None] * 5, {**reports, (1, 3): None, (4, 0): None})
        assert len(out) == 4 and all(set(d) == edges for d in out)
        assert all(out[0][e] is rot[e] and out[3][e] is reports[e] for e in edges)
    # a tighter and a looser threshold move the decision on the 15 degree triplet
    assert CycleConsistentRotationViewGraphEstimator("MEDIAN_EDGE_ERROR", error_threshold=16.0).run(
        rot, i2Ui1, [], corr, [], reports) == set(ref.REFERENCE_SCENE_EDGES)
