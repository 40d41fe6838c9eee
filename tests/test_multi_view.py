"""CPU: pins the restatement of gtsfm_assemble_ba_input (tests/multi_view_ref.py assemble_ref) on hand-written cases,
against networkx where it imports, and the binding of the new entry point."""
import itertools
import os
import re

import numpy as np
import pytest

from tests import multi_view_ref as M
from tests.conftest import REPO

CASES = M.hand_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_assemble_ref_hand_cases(name):
    case, cam_keep, track_keep, track_len, stats = CASES[name]
    r = M.run_case(case)
    assert r.cam_keep.tolist() == cam_keep
    assert r.track_keep.tolist() == track_keep
    assert r.track_len.tolist() == track_len
    assert r.stats.tolist() == stats


def _networkx_cameras(case):
    """get_nodes_in_largest_connected_component's logic (gtsfm/utils/graph.py:29-39) on the camera edges of
    select_largest_connected_component (gtsfm/common/gtsfm_data.py:250-266), rebuilt from nx.Graph calls."""
    import networkx as nx

    off, img, inl = case["offsets"], case["img"], case["inlier"]
    edges = []
    for t in range(len(off) - 1):
        if case["track_valid"][t]:
            cams = [int(img[m]) for m in range(off[t], off[t + 1]) if inl[m]]
            edges += list(itertools.combinations(cams, 2))
    if case["extra_edges"] is not None:
        edges += [(int(a), int(b)) for a, b in case["extra_edges"]
                  if 0 <= a < case["n_img"] and 0 <= b < case["n_img"] and case["cam_valid"][a] and case["cam_valid"][b]]
    if len(edges) == 0:
        return []
    g = nx.Graph()
    g.add_edges_from(edges)
    largest_cc = max(nx.connected_components(g), key=len)
    return list(g.subgraph(largest_cc).copy().nodes())


def _check_against_networkx(case):
    nodes = _networkx_cameras(case)
    want = np.array([bool(case["cam_valid"][i]) and i in nodes for i in range(case["n_img"])], np.uint8)
    np.testing.assert_array_equal(M.run_case(case).cam_keep, want)


@pytest.mark.parametrize("name", sorted(CASES))
def test_assemble_ref_equals_networkx(name):
    pytest.importorskip("networkx")
    _check_against_networkx(CASES[name][0])


def test_assemble_ref_equals_networkx_random_ties():
    """Many equal-size components: the tie rule (first contributing item) is the one networkx applies."""
    pytest.importorskip("networkx")
    rng = np.random.default_rng(11)
    for _ in range(40):
        _check_against_networkx(M.random_case(rng, n_img=64, n_tracks=60))
    for _ in range(40):  # disjoint pairs of cameras in a random order: every component has two cameras
        cams = rng.permutation(32).reshape(-1, 2)
        n_extra = int(rng.integers(0, 4))
        case = M.pack_case([list(map(int, p)) for p in cams[n_extra:]], 32,
                           extra_edges=cams[:n_extra] if n_extra else None)
        _check_against_networkx(case)


def test_init_cameras_ref():
    wRi = np.tile(2.0 * np.eye(3), (3, 1, 1))
    c = M.init_cameras_ref(wRi, np.ones((3, 3)), [1, 0, 1], np.tile([500.0, 1.0, 2.0], (3, 1)))
    assert c.valid.tolist() == [True, False, True]
    np.testing.assert_array_equal(c.wRc[1], np.eye(3))
    np.testing.assert_array_equal(c.wtc, [[1, 1, 1], [0, 0, 0], [1, 1, 1]])
    np.testing.assert_array_equal(c.wRc[0], 2.0 * np.eye(3))


def test_binding_carries_assemble_ba_input():
    """The binding table holds both new functions with the header's parameter counts, the library exports them, and
    the query answers without a GPU."""
    from gtsfm_amd import native

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "gtsfm_hip.h")).read(), flags=re.S)
    for name in ("gtsfm_assemble_ba_input_workspace_bytes", "gtsfm_assemble_ba_input"):
        params = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, text, flags=re.S).group(1)
        assert name in native.SIGNATURES
        assert len(native.SIGNATURES[name][1]) == params.count(",") + 1
        assert hasattr(native.lib(), name)
    assert len(native.BA_INPUT_STATS_FIELDS) == 6
    L = native.lib()
    assert L.gtsfm_assemble_ba_input_workspace_bytes(300, 64) > 0
    assert L.gtsfm_assemble_ba_input_workspace_bytes(0, 64) == 0 and L.gtsfm_assemble_ba_input_workspace_bytes(3, 0) == 0
    assert L.gtsfm_assemble_ba_input_workspace_bytes(300, 64) < L.gtsfm_assemble_ba_input_workspace_bytes(3000, 64)


def test_assemble_metrics():
    from gtsfm_amd.data_association.data_assoc import assemble_metrics

    m = assemble_metrics(np.array([2, 9, 30, 100, 40, 12], np.int64), 60)
    assert m == {"accepted_tracks_ratio": 0.5, "num_accepted_tracks": 30, "number_cameras": 9}


def test_multi_view_optimizer_module():
    """The chain's public names exist and pose priors are refused before the GPU is touched."""
    from gtsfm_amd import multi_view_optimizer as mvo

    opt = mvo.MultiViewOptimizer(None, None, None, None)
    assert opt.view_graph_estimator is None and not opt._run_view_graph_estimator
    with pytest.raises(NotImplementedError):
        opt.run(2, [None, None], {}, {}, {}, [None, None], relative_pose_priors={(0, 1): object()})
    assert mvo.MultiViewArrays._fields == ("keep", "rotations", "tracks", "translations", "cameras", "triangulated",
                                           "valid", "ba_input", "ba")
