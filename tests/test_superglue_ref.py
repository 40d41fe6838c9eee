"""The reference side of tests/test_superglue_edges_gpu.py, on the CPU: oracle.deep.superglue in float32 against the
same restatement in float64 at every shape the GPU suite runs, so that the GPU bars (log-assignment within 2e-3,
differing matches capped at max(2, 2 %)) are known to leave room for the kernel: float32 arithmetic alone, in torch's
summation order, stays within 5e-4 and within the match cap on the seeds of tests/superglue_cases.py. The measured
figures are printed and kept in superglue_cases.MEASURED. The float64 restatement itself is pinned to the reference
module's golden log-assignment matrix.
"""
import functools
import os

import numpy as np
import pytest

import superglue_cases as sc
from superpoint_weights import superglue_state_dict
from tests.conftest import GOLDEN


@functools.lru_cache(maxsize=None)
def _sd():
    return superglue_state_dict(0)


def _cases():
    out = {f"{n0}x{n1}": (lambda n0=n0, n1=n1: sc.make_pair(n0, n1)) for n0, n1 in sc.SHAPES}
    out["128x129_hw_swapped"] = lambda: sc.make_pair(128, 129, sc.HW1, sc.HW0)
    for i, j in sc.SHARED_PAIRS:
        out[f"shared_{i}_{j}"] = lambda i=i, j=j: tuple(
            sc.make_images(sc.SHARED_COUNTS, sc.SHARED_HW, sc.SHARED_SEED)[k] for k in (i, j))
    out["pad_150x170"] = lambda: sc.make_pair(*sc.BIG_PAD_SHAPE)
    out["big_2112x2050"] = lambda: sc.make_pair(*sc.BIG_SHAPE)
    return out


CASES = _cases()


def test_measured_table_is_complete():
    assert set(sc.MEASURED) == set(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_float32_restatement_within_quarter_of_gpu_bar(name):
    a, b = CASES[name]()
    m64, s64, Z64 = sc.reference(a, b, _sd(), "float64")
    m32, s32, Z32 = sc.reference(a, b, _sd(), "float32")
    assert Z64.dtype == np.float64 and Z32.dtype == np.float32 and Z64.shape == (len(a.kp) + 1, len(b.kp) + 1)
    live = Z64 > -20
    dz = float(np.abs(Z32[live] - Z64[live]).max())
    ds = float(np.abs(s32 - s64).max())
    nd, nref = int((m32 != m64).sum()), int((m64 >= 0).sum())
    print(f'    "{name}": ({dz:.2e}, {ds:.2e}, {nd}, {nref}),')
    assert dz <= 5e-4, (name, dz)
    assert (Z32[~live] < -15).all()
    assert nd <= max(2, 0.02 * nref), (name, nd, nref)
    if min(len(a.kp), len(b.kp)) >= 63:
        assert nref >= 5, (name, nref)


def test_float64_restatement_reproduces_golden_log_assignment():
    """The float64 restatement against the reference module's own float32 log-assignment matrix of small_150x170
    (tests/golden/superglue_random_w0.npz): within 1e-4 everywhere, matches identical."""
    import torch

    from oracle import deep

    g = np.load(os.path.join(GOLDEN, "superglue_random_w0.npz"))
    k = lambda n: g[f"small_150x170__{n}"]  # noqa: E731
    hw = tuple(int(v) for v in k("hw"))
    m0, ms0, Z = deep.superglue(k("kp0"), k("kp1"), k("d0"), k("d1"), k("s0"), k("s1"), hw, hw, _sd(),
                                return_log_assignment=True, dtype=torch.float64)
    d = float(np.abs(Z - k("Z")).max())
    print(f"float64 restatement vs golden Z: {d:.2e}")
    assert Z.shape == k("Z").shape and d <= 1e-4
    np.testing.assert_array_equal(m0, k("matches0"))
    np.testing.assert_allclose(ms0, k("mscores0"), atol=1e-4)


def test_defaults_unchanged():
    """Without the new options the restatement returns the float32 pair it always did, bit for bit the float32 run
    with the matrix asked for."""
    from oracle import deep

    a, b = sc.make_pair(15, 17)
    m, s = deep.superglue(a.kp, b.kp, a.desc, b.desc, a.scores, b.scores, a.hw, b.hw, _sd())
    m2, s2, Z = sc.reference(a, b, _sd(), "float32")
    assert s.dtype == np.float32 and Z.dtype == np.float32
    np.testing.assert_array_equal(m, m2)
    np.testing.assert_array_equal(s, s2)
