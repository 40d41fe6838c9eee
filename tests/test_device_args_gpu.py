"""GPU: the argument handling every gtsfm_amd.device wrapper shares -- the tensor check, the workspace rule and the
track-CSR preamble -- on the smallest inputs that reach each branch.

The workspace rule: a caller's buffer is used when it holds the queried bytes, else the call allocates its own
(device._workspace is counted to tell the two apart); either way, and on a side stream, the results are those of
workspace=None. A failed tensor check raises AssertionError naming the argument before the library is touched
(native.lib is replaced by a stand-in whose every attribute access fails).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
EDGES = np.array([[0, 1], [0, 2], [1, 2]], np.int32)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class _NoLibrary:
    def __getattr__(self, name):
        raise RuntimeError(f"the library was reached: {name}")


@pytest.fixture
def no_library(monkeypatch):
    from gtsfm_amd import native

    monkeypatch.setattr(native, "lib", lambda: _NoLibrary())


@pytest.fixture
def fresh_workspaces(monkeypatch):
    """The sizes device._workspace was asked for."""
    from gtsfm_amd import device

    asked, real = [], device._workspace

    def counted(nbytes, dev):
        asked.append(int(nbytes))
        return real(nbytes, dev)

    monkeypatch.setattr(device, "_workspace", counted)
    return asked


def _cycle_filter(**kw):
    from gtsfm_amd import device, native

    R = _t(np.tile(np.eye(3), (3, 1, 1)))
    return device.viewgraph_cycle_filter(_t(EDGES), R, None, 3, native.GTSFM_VG_MIN_EDGE_ERROR, 7.0, **kw)


def test_workspace_none_small_exact_and_side_stream_agree(fresh_workspaces):
    from gtsfm_amd import native

    need = int(native.lib().gtsfm_viewgraph_workspace_bytes(3, 3))
    assert need > 16
    base = _cycle_filter()
    assert fresh_workspaces == [need]
    small = _cycle_filter(workspace=torch.empty(16, dtype=torch.uint8, device=DEV))
    assert fresh_workspaces == [need, need]  # 16 bytes do not hold it: the call allocated its own
    exact = _cycle_filter(workspace=torch.empty(need, dtype=torch.uint8, device=DEV))
    assert fresh_workspaces == [need, need]  # the caller's buffer was used
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    streamed = _cycle_filter(stream=side)
    side.synchronize()
    keep, agg, n_trip, total = (x.cpu() for x in base)
    assert keep.tolist() == [1, 1, 1] and n_trip.tolist() == [1, 1, 1] and int(total[0]) == 1
    assert agg.abs().max() < 1e-9  # identity rotations close every cycle
    for other in (small, exact, streamed):
        for a, b in zip(base, other):
            assert a.dtype == b.dtype and torch.equal(a.cpu(), b.cpu())


def test_cycle_filter_names_the_bad_argument(no_library):
    from gtsfm_amd import device, native

    R = _t(np.tile(np.eye(3), (3, 1, 1)))
    args = (3, native.GTSFM_VG_MIN_EDGE_ERROR, 7.0)
    with pytest.raises(AssertionError, match="edges"):
        device.viewgraph_cycle_filter(_t(EDGES.astype(np.int64)), R, None, *args)
    strided = _t(np.tile(np.eye(3), (6, 1, 1)))[::2]
    assert strided.numel() == 27 and not strided.is_contiguous()
    with pytest.raises(AssertionError, match=r"\bR\b"):
        device.viewgraph_cycle_filter(_t(EDGES), strided, None, *args)
    with pytest.raises(AssertionError, match="valid"):
        device.viewgraph_cycle_filter(_t(EDGES), R, _t(np.ones(2, np.uint8)), *args)


def test_sampson_names_F(no_library):
    from gtsfm_amd import device

    x = _t(np.zeros((1, 2)))
    with pytest.raises(AssertionError, match=r"\bF\b"):
        device.sampson_sq(_t(np.eye(3, dtype=np.float32)[None]), _t(np.zeros(1, np.int32)), x, x)


def _rot(axis, angle):
    k = np.zeros(3)
    k[axis] = 1.0
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def test_rotavg_replaces_a_small_workspace(fresh_workspaces):
    """A caller's workspace below the queried size is replaced (the rule of every other wrapper) and the result is
    that of workspace=None, bit for bit."""
    from gtsfm_amd import device, native

    wR = [np.eye(3), _rot(2, 0.3), _rot(0, 0.5) @ _rot(1, -0.2)]
    aRb = np.stack([wR[a].T @ wR[b] for a, b in EDGES])  # wRa aRb = wRb
    base = device.rotavg_shonan(_t(EDGES), _t(aRb), None, None, 3)
    small = device.rotavg_shonan(_t(EDGES), _t(aRb), None, None, 3,
                                 workspace=torch.empty(16, dtype=torch.uint8, device=DEV))
    assert len(fresh_workspaces) == 2 and fresh_workspaces[0] == fresh_workspaces[1] > 16
    assert int(base.stats.cpu()[11]) == native.RA_STATUS_CERTIFIED and base.rot_valid.cpu().tolist() == [1, 1, 1]
    for a, b in ((base.wRi, small.wRi), (base.rot_valid, small.rot_valid), (base.stats, small.stats)):
        assert torch.equal(a.cpu(), b.cpu())


def _empty_csr():
    cams = (_t(np.tile(np.eye(3), (2, 1, 1))), _t(np.zeros((2, 3))), _t(np.tile([500.0, 320.0, 240.0], (2, 1))))
    return (_t(np.zeros(0, np.int32)), _t(np.zeros(0, np.int32)), _t(np.zeros((0, 2), np.float32))), cams


def test_triangulate_refuses_an_empty_track_offsets(no_library):
    from gtsfm_amd import device, native

    csr, cams = _empty_csr()
    with pytest.raises(AssertionError, match="track_offsets"):
        device.triangulate_tracks(*csr, *cams, None, native.GTSFM_TRI_NO_RANSAC, 3.0)


def test_global_ba_takes_an_empty_track_offsets_as_no_tracks():
    """The wrapper takes an empty track_offsets as T = 0 (no AssertionError, unlike triangulate_tracks) and calls the
    library. The library then does not report GBA_STATUS_NOTHING for it: gtsfm_global_ba refuses the null pointers
    of the zero-sized point / track_keep outputs with GTSFM_ERR_ARG before it looks at the counts. Measured on the
    commit before the wrappers shared their checks and after it: NativeError with status -1 both times, which is
    what this asserts."""
    from gtsfm_amd import device, native

    csr, cams = _empty_csr()
    with pytest.raises(native.NativeError, match="gtsfm_global_ba failed with status -1"):
        device.global_ba(*csr, _t(np.zeros((0, 3))), None, None, *cams, None)
