"""CPU: pins the numpy restatement of Shonan rotation averaging (tests/rotation_averaging_ref.py) to the reference's own
expectations (tests/averaging/rotation/test_shonan.py and tests/data/sample_poses.py, whose numbers live under
tests/golden/rotation_averaging/), checks the saddle escape of the staircase, measures the floor the GPU test scales
its tolerances from, and checks the Python surface that needs no GPU."""
import pickle

import numpy as np
import pytest

from tests import rotation_averaging_ref as ref

ROTATION_ANGLE_ERROR_THRESHOLD_DEG = 2.0  # test_shonan.py
# The restatement against itself, (a) with another seed and (b) with its gradient tolerance tightened 100 times, over
# every case of this file and of the GPU file: the larger difference, measured 5.7e-8 degrees, 1.6e-11 in the final
# cost and 2.3e-11 in lambda_min (solver tolerance, not rounding). tests/test_rotation_averaging_gpu.py allows 10 x.
ROTATION_FLOOR_DEG = 6e-8
COST_FLOOR = 2e-11
EIGENVALUE_FLOOR = 3e-11

CASES = {
    "circle_two_edges": lambda: ref.golden("circle_two_edges"), "circle_all_edges": lambda: ref.golden("circle_all_edges"),
    "line_large_edges": lambda: ref.golden("line_large_edges"), "panorama": lambda: ref.golden("panorama"),
    "simple": ref.simple, "simple_with_prior": ref.simple_with_prior, "nonconsecutive": ref.nonconsecutive,
    "skydio32": lambda: ref.golden("skydio32"), "ring6": ref.ring6,
}
SCENES = {"scene40": lambda: ref.seeded_scene(40, 5), "scene40_two_components": lambda: ref.seeded_scene(40, 5, extra_component=3),
          "hub300": ref.hub_scene}
THRESHOLD_DEG = {"nonconsecutive": 0.1}


@pytest.fixture(scope="module")
def solved():
    out = {}
    for name, make in {**CASES, **SCENES}.items():
        c = make()
        out[name] = (c, ref.run_case(c))
    return out


@pytest.mark.parametrize("name", [n for n in CASES if n != "ring6"])
def test_reference_cases(solved, name):
    c, r = solved[name]
    assert r.stats[11] == 0 and r.stats[2] == 5, "certified at p = 5"
    assert r.stats[3] > -1e-4
    assert np.array_equal(r.rot_valid.astype(bool), c["expected_valid"])
    ang = ref.aligned_angles_deg(c["expected"], r.wRi, c["expected_valid"])
    print(name, "max angle after alignment, degrees:", ang.max(), "cost", r.stats[1], "lambda_min", r.stats[3])
    assert ang.max() <= THRESHOLD_DEG.get(name, ROTATION_ANGLE_ERROR_THRESHOLD_DEG)


def test_nonconsecutive_camera_zero_is_invalid(solved):
    _, r = solved["nonconsecutive"]
    assert r.rot_valid.tolist() == [0, 1, 1, 1] and not r.wRi[0].any()


def test_ring_start_is_a_saddle():
    c = ref.ring6()
    P = ref.build_problem(c["edges"], c["aRb"], c["kappa"], None, 6)
    Y = c["wRi_init"].copy()
    G = ref.apply_Q(P, Y)
    Lam = ref.lambda_blocks(Y, G)
    assert abs(np.sum(Y * G) - 12.0) < 1e-12
    assert np.abs(2.0 * (G - Y @ Lam)).max() < 1e-14
    w = np.linalg.eigvalsh(ref.dense_S(P, Lam))
    assert abs(w[0] + 1.0) < 1e-12 and abs(w[1] + 1.0) < 1e-12 and w[2] > -1e-12


def test_ring_escapes_the_saddle(solved):
    c, r = solved["ring6"]
    print("ring: final p", r.stats[2], "cost", r.stats[1], "lambda_min", r.stats[3])
    assert r.stats[0] == pytest.approx(12.0, abs=1e-12)
    assert r.stats[11] == 0 and r.stats[2] >= 4
    assert r.stats[1] < 1e-9
    assert ref.aligned_angles_deg(c["expected"], r.wRi).max() < 1e-6


def test_largest_component_and_invalid_edge():
    c = ref.seeded_scene(40, 5, extra_component=3)
    P = ref.build_problem(c["edges"], c["aRb"], c["kappa"], None, c["n_img"])
    assert P.n == 40 and not P.keep[40:].any()
    ev = np.ones(len(c["edges"]), np.uint8)
    ev[7] = 0
    assert len(ref.build_problem(c["edges"], c["aRb"], c["kappa"], ev, c["n_img"]).a) == len(P.a) - 1


def test_restatement_floor(solved):
    """The floor of tests/test_rotation_averaging_gpu.py: the restatement against itself with another seed and with
    its gradient tolerance tightened 100 times."""
    rot = cost = eig = 0.0
    for name, (c, r0) in solved.items():
        for kw in (dict(seed=1), dict(grad_rel_tol=ref.DEFAULTS["grad_rel_tol"] / 100)):
            r = ref.run_case(c, **kw)
            assert r.stats[11] == r0.stats[11] == 0 and r.stats[2] == r0.stats[2]
            rot = max(rot, ref.aligned_angles_deg(r0.wRi, r.wRi, r0.rot_valid).max())
            cost = max(cost, abs(r.stats[1] - r0.stats[1]))
            eig = max(eig, abs(r.stats[3] - r0.stats[3]))
    print("floor: rotations %.3g degrees, cost %.3g, lambda_min %.3g" % (rot, cost, eig))
    assert rot <= ROTATION_FLOOR_DEG and cost <= COST_FLOOR and eig <= EIGENVALUE_FLOOR
    assert 10 * ROTATION_FLOOR_DEG < 0.01


def test_alignment_helper():
    rng = np.random.default_rng(0)
    A = np.array([ref.rodrigues(rng.normal(size=3)) for _ in range(5)])
    Rg = ref.rodrigues(np.array([0.3, -1.0, 2.0]))
    assert ref.aligned_angles_deg(A, Rg.T @ A).max() < 1e-12


def test_abi_and_symbols():
    from gtsfm_amd import native

    assert native.ABI_VERSION == 407 and native.lib().gtsfm_hip_abi_version() == 407
    L = native.lib()
    for name in ("gtsfm_rotavg_workspace_bytes", "gtsfm_rotavg_shonan"):
        assert name in native.SIGNATURES and hasattr(L, name)
    assert len(native.RA_STATS_FIELDS) == 12
    assert L.gtsfm_rotavg_workspace_bytes(43, 32, 30) > 0
    assert L.gtsfm_rotavg_workspace_bytes(43, 32, 31) == 0 and L.gtsfm_rotavg_workspace_bytes(0, 32, 30) == 0
    assert L.gtsfm_rotavg_workspace_bytes(43, 32, 5) < L.gtsfm_rotavg_workspace_bytes(43, 32, 30)


def test_class_surface():
    from gtsfm_amd.averaging.rotation import RotationAveragingBase, ShonanRotationAveraging

    obj = ShonanRotationAveraging(two_view_rotation_sigma=0.5)
    assert isinstance(obj, RotationAveragingBase)
    clone = pickle.loads(pickle.dumps(obj))
    assert type(clone) is type(obj) and clone.__dict__ == obj.__dict__
    assert (clone._p_min, clone._p_max, clone._two_view_rotation_sigma) == (5, 30, 0.5)
    assert obj.run_rotation_averaging(4, {}, {}) == [None] * 4  # shonan.py:178-181, no GPU needed
    assert obj.run_rotation_averaging(2, {(0, 1): None}, {}) == [None] * 2
