"""GPU: holds gtsfm_rotavg_shonan (gtsfm_amd/csrc/rotavg.hip) to the numpy restatement
(tests/rotation_averaging_ref.py): status, final level and the sign of the certificate exactly; rotations (after
alignment: the optimum is unique up to gauge), final cost and lambda_min within ten times the floor that
tests/test_rotation_averaging.py measures on the restatement itself."""
import json
import os

import numpy as np
import pytest
import torch

from tests import rotation_averaging_ref as ref
from tests.conftest import GOLDEN
from tests.test_rotation_averaging import (CASES, COST_FLOOR, EIGENVALUE_FLOOR, ROTATION_ANGLE_ERROR_THRESHOLD_DEG,
                                           ROTATION_FLOOR_DEG, SCENES, THRESHOLD_DEG)

pytestmark = pytest.mark.gpu

ROTATION_CEILING_DEG = 10 * ROTATION_FLOOR_DEG
COST_CEILING = 10 * COST_FLOOR
EIGENVALUE_CEILING = 10 * EIGENVALUE_FLOOR


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda:0"))


def _run(c, **kw):
    from gtsfm_amd import device

    kw.setdefault("p_min", c["p_min"])
    ev = c.get("edge_valid")
    return device.rotavg_shonan(_t(c["edges"].astype(np.int32)), _t(c["aRb"]), _t(c["kappa"]),
                                None if ev is None else _t(np.asarray(ev, np.uint8)), c["n_img"], _t(c["wRi_init"]), **kw)


@pytest.fixture(scope="module")
def restated():
    cache = {}

    def get(name, c):
        if name not in cache:
            cache[name] = ref.run_case(c)
        return cache[name]

    return get


def _compare(name, c, got, want):
    stats = got.stats.cpu().numpy()
    wRi, ok = got.wRi.cpu().numpy(), got.rot_valid.cpu().numpy()
    print(name, "gpu stats", stats.tolist())
    print(name, "ref stats", want.stats.tolist())
    assert stats[11] == want.stats[11] and stats[2] == want.stats[2]
    assert (stats[3] > -1e-4) == (want.stats[3] > -1e-4)
    assert stats[9] == want.stats[9] and stats[10] == want.stats[10]
    np.testing.assert_array_equal(ok, want.rot_valid)
    assert not wRi[ok == 0].any()
    ang = ref.aligned_angles_deg(want.wRi, wRi, ok).max()
    dcost, deig = abs(stats[1] - want.stats[1]), abs(stats[3] - want.stats[3])
    print(name, "rotations %.3g degrees, cost %.3g, lambda_min %.3g, eigen residual %.3g, Lanczos steps %d" %
          (ang, dcost, deig, stats[4], stats[8]))
    assert abs(stats[0] - want.stats[0]) <= 1e-12 * max(1.0, want.stats[0])
    assert ang <= ROTATION_CEILING_DEG
    assert dcost <= COST_CEILING
    assert deig <= EIGENVALUE_CEILING
    assert stats[4] <= 1e-8
    R = wRi[ok == 1]
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-13 and np.allclose(np.linalg.det(R), 1.0)
    return wRi, ok, stats


@pytest.mark.parametrize("name", list(CASES))
def test_reference_cases(restated, name):
    c = CASES[name]()
    wRi, ok, stats = _compare(name, c, _run(c), restated(name, c))
    ang = ref.aligned_angles_deg(c["expected"], wRi, c["expected_valid"])
    assert np.array_equal(ok.astype(bool), c["expected_valid"])
    assert ang.max() <= THRESHOLD_DEG.get(name, ROTATION_ANGLE_ERROR_THRESHOLD_DEG)
    if name == "ring6":
        assert stats[0] == pytest.approx(12.0, abs=1e-12) and stats[2] >= 4 and stats[1] < 1e-9


def test_scene40_with_cleared_edge(restated):
    c = SCENES["scene40"]()
    c["edge_valid"] = np.ones(len(c["edges"]), np.uint8)
    c["edge_valid"][7] = 0
    _, _, stats = _compare("scene40 / cleared edge", c, _run(c), restated("scene40_cleared", c))
    assert stats[10] == len(c["edges"]) - 1


def test_scene40_second_component_is_invalid(restated):
    c = SCENES["scene40_two_components"]()
    _, ok, stats = _compare("scene40 / two components", c, _run(c), restated("scene40_two", c))
    assert ok[:40].all() and not ok[40:].any() and stats[9] == 40


def test_hub_row_spans_waves(restated):
    c = SCENES["hub300"]()
    assert np.bincount(c["edges"].ravel())[0] == 299 > 256
    _compare("hub300", c, _run(c), restated("hub300", c))


def test_two_calls_same_bytes():
    c = SCENES["scene40"]()
    a, b = _run(c), _run(c)
    assert np.array_equal(a.wRi.cpu().numpy().view(np.uint64), b.wRi.cpu().numpy().view(np.uint64))
    assert np.array_equal(a.stats.cpu().numpy().view(np.uint64), b.stats.cpu().numpy().view(np.uint64))
    assert np.array_equal(a.rot_valid.cpu().numpy(), b.rot_valid.cpu().numpy())


def test_argument_checks():
    from gtsfm_amd import native

    c = ref.simple()
    for kw in (dict(p_min=2), dict(p_min=6, p_max=5), dict(p_max=31)):
        with pytest.raises(native.NativeError, match="status -1|unsupported"):
            _run(c, **kw)
    L = native.lib()
    e, R = _t(c["edges"].astype(np.int32)), _t(c["aRb"])
    out = torch.empty((3, 3, 3), dtype=torch.float64, device=e.device)
    ok = torch.empty(3, dtype=torch.uint8, device=e.device)
    st = torch.empty(12, dtype=torch.float64, device=e.device)
    need = L.gtsfm_rotavg_workspace_bytes(2, 3, 30)
    ws = torch.empty(need, dtype=torch.uint8, device=e.device)

    def call(edges, nbytes):
        return L.gtsfm_rotavg_shonan(edges, R.data_ptr(), None, None, 2, 3, None, 0, 5, 30, -1e-4, 1e-10, 100, 1e-2, 200,
                                     1e-8, 4000, ws.data_ptr(), nbytes, out.data_ptr(), ok.data_ptr(), st.data_ptr(),
                                     native.stream_handle())

    assert call(None, need) == native.GTSFM_ERR_ARG
    assert call(e.data_ptr(), need - 1) == native.GTSFM_ERR_CAPACITY
    assert call(e.data_ptr(), need) == native.GTSFM_OK and st.cpu()[11] == 0


def test_plugin_and_chain_into_translation_averaging():
    """circle_all_edges of tests/golden/translation_averaging: rotations averaged from i2Ri1 = wRi2' wRi1, aligned to
    the fixture's frame, then the existing translation averaging, held to the existing circle test's expectation."""
    from gtsfm_amd.averaging.rotation import ShonanRotationAveraging
    from gtsfm_amd.averaging.translation import TranslationAveraging1DSFM
    from tests import translation_averaging_ref as ta_ref
    from tests import translation_averaging_scenes as scenes
    from tests.test_translation_averaging import ABSOLUTE_ERROR_THRESHOLD, RELATIVE_ERROR_THRESHOLD

    case = scenes.sample_case("circle_all_edges")
    edges, wRi = np.asarray(case["edges"], np.int32), np.asarray(case["wRi"], np.float64)
    i2Ri1 = np.array([wRi[i2].T @ wRi[i1] for i1, i2 in edges])
    rot = ShonanRotationAveraging().run_rotation_averaging_arrays(_t(edges), _t(i2Ri1), None, len(wRi))
    assert rot.stats[11].item() == 0 and rot.rot_valid.all()
    aligned = ref.align(wRi, rot.wRi.cpu().numpy())
    assert ref.angles_deg(wRi, aligned).max() < 1e-6
    res = TranslationAveraging1DSFM().run_translation_averaging_arrays(_t(edges), _t(case["i2Ui1"]), _t(aligned), None,
                                                                       rot.rot_valid)
    assert res.stats[9].item() == 0 and res.wti_valid.all()
    got = ta_ref.align_sim3(case["wti"], res.wti.cpu().numpy())
    assert np.allclose(got, case["wti"], atol=ABSOLUTE_ERROR_THRESHOLD, rtol=1e-1)
    extent = max(np.linalg.norm(case["wti"] - case["wti"].mean(0), axis=1).max(), 1.0)
    assert np.abs(got - case["wti"]).max() <= RELATIVE_ERROR_THRESHOLD * extent
    # the reference's signature, with a non-consecutive graph: camera 0 has no measurement
    c = ref.nonconsecutive()
    out = ShonanRotationAveraging().run_rotation_averaging(4, {tuple(p): R for p, R in zip(c["pairs"].tolist(), c["aRb"])}, {})
    assert out[0] is None and all(o is not None for o in out[1:])
    from gtsfm_amd.common import geometry

    got_R = np.array([np.eye(3)] + [geometry.rotation_matrix(o) for o in out[1:]])
    assert ref.aligned_angles_deg(c["expected"], got_R, c["expected_valid"]).max() <= 0.1
