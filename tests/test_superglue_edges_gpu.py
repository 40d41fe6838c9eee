"""HIP SuperGlue (gtsfm_superglue_batched) against the float64 restatement (oracle.deep.superglue, dtype float64) where
the three golden shapes of tests/test_superglue_gpu.py never go. Weights: superglue_state_dict(0). Inputs are generated
by tests/superglue_cases.py; tests/test_superglue_ref.py shows that float32 arithmetic alone stays within 5e-4 of this
reference on the same seeds (superglue_cases.MEASURED), a quarter of the bar below.

Bars (tests/test_superglue_gpu.py's): log-assignment Z within 2e-3 absolute where the reference is > -20 and below
-15 elsewhere; matching_scores0 within 2e-3 (*); matches identical except at near-ties (row, column or threshold margin
below 4e-3 on the GPU's own Z), at most max(2, 2 %) of the reference's matches differing.

(*) matching_scores0 is exp(Z) of the mutual row maxima: a probability after any Sinkhorn iteration, where the bar is
the absolute 2e-3. With sinkhorn_iters = 0 nothing is normalised and exp(Z) reaches 1e25 on these inputs (the float32
restatement alone is 3e20 away from the float64 one there), so above 1 the same bar is taken relative,
|ds| <= 2e-3 max(1, s_ref): what Z within 2e-3 implies for exp(Z).

Which test reaches which path:
1. production two-pass Sinkhorn (sk_rows_kernel / sk_cols_kernel, kmax 2112 > kSkFusedMaxK, nine attention query
   blocks): test_two_pass_dispatch_and_heavy_padding.
2. kmax 64 and 128 (M below one GEMM tile, one partly filled attention workgroup and a single key chunk, one or two
   sk_pass_kernel blocks): test_single_pair_table at (1,1) ... (64,64) and (65,127) ... (128,127).
3. counts at and next to 16 / 64 / 128 / 256 and below 16, the dustbin row alone in a row block (m = 64, 128, 256) or
   the dustbin column in lane 0 of the next column group (n = 64, 128): test_single_pair_table.
4. per-side image size: every table pair has hw0 != hw1; test_hw_is_per_side swaps them.
5. an image in several pairs and on both sides: test_shared_images.
6. a small pair padded beside a 2112-row pair: test_two_pass_dispatch_and_heavy_padding.
7. n_layers, sinkhorn_iters, match_threshold off their defaults: test_parameters.
8. the entry point's own checks and a zero-count side: test_entry_point_checks, test_zero_count_side.
9. superglue_pairs_batched's chunking: test_chunked_equals_unchunked.
"""
import functools

import numpy as np
import pytest
import torch

import superglue_cases as sc
from superpoint_weights import superglue_state_dict

pytestmark = pytest.mark.gpu
Z_ATOL, DEAD, SCORE_ATOL, TIE = 2e-3, -15.0, 2e-3, 4e-3


@functools.lru_cache(maxsize=None)
def _sd():
    return superglue_state_dict(0)


@functools.lru_cache(maxsize=None)
def _weights(n_layers=18):
    from gtsfm_amd import native
    from gtsfm_amd.frontend.matcher.superglue_matcher import SuperGlueMatcher

    native.require_gpu()
    return SuperGlueMatcher(state_dict=_sd(), n_layers=n_layers).weights()


@functools.lru_cache(maxsize=None)
def _table_ref(n0, n1):
    a, b = sc.make_pair(n0, n1)
    return a, b, sc.reference(a, b, _sd())


@functools.lru_cache(maxsize=None)
def _shared():
    imgs = sc.make_images(sc.SHARED_COUNTS, sc.SHARED_HW, sc.SHARED_SEED)
    return imgs, [sc.reference(imgs[i], imgs[j], _sd()) for i, j in sc.SHARED_PAIRS]


def _compare(what, run, q, ref, thr=0.2, rows=None):
    """Pair q of `run` against ref = (matches0, mscores0, Z) of the float64 restatement: prints the measured maxima,
    then holds them to the bars. rows: compare only these rows of Z."""
    m_ref, s_ref, Z_ref = ref
    Z = run.Z[q]
    assert Z.shape == Z_ref.shape and Z.dtype == np.float32
    n0, n1 = Z.shape[0] - 1, Z.shape[1] - 1
    zg, zr = (Z, Z_ref) if rows is None else (Z[rows], Z_ref[rows])
    live = zr > -20
    dz = float(np.abs(zg[live] - zr[live]).max())
    dead = float(zg[~live].max()) if (~live).any() else -np.inf
    ds = float((np.abs(run.mscores0[q] - s_ref) / np.maximum(1.0, s_ref)).max())  # absolute wherever s_ref <= 1
    nref = int((m_ref >= 0).sum())
    margins = sc.near_tie_margins(Z[:n0, :n1], run.matches0[q], m_ref, thr)
    print(f"{what}: |dZ| {dz:.2e} (live {int(live.sum())}, max dead {dead:.1f}), |dscore| {ds:.2e}, "
          f"differing {len(margins)} of {nref} matches, largest near-tie margin "
          f"{max(margins.values()) if margins else 0.0:.2e}")
    assert np.isfinite(zg).all()
    assert dz <= Z_ATOL, (what, dz)
    assert dead < DEAD, (what, dead)
    assert ds <= SCORE_ATOL, (what, ds)
    assert len(margins) <= max(2, 0.02 * max(nref, 1)), (what, len(margins), nref)
    assert all(v < TIE for v in margins.values()), (what, margins)
    pr = run.pairs_out[q]
    assert pr.dtype == np.uint32 and np.all(np.diff(pr[:, 0].astype(np.int64)) > 0)


def _same(a, b, q, r=0):
    """Pair q of run a is bit for bit pair r of run b."""
    np.testing.assert_array_equal(a.Z[q], b.Z[r])
    np.testing.assert_array_equal(a.pairs_out[q], b.pairs_out[r])
    np.testing.assert_array_equal(a.mscores0[q], b.mscores0[r])


@pytest.mark.parametrize("n0,n1", sc.SHAPES)
def test_single_pair_table(n0, n1):
    a, b, ref = _table_ref(n0, n1)
    run = sc.run_gpu([a, b], [(0, 1)], _weights())
    assert run.kmax == (max(n0, n1) + 63) // 64 * 64
    _compare(f"{n0}x{n1}", run, 0, ref)


def test_hw_is_per_side():
    """(128, 129) with the two image sizes exchanged: the reference itself moves by more than the bar, so a kernel
    that used one side's size for both, or the other side's, fails one of the two arrangements."""
    a, b, ref = _table_ref(128, 129)
    a2, b2 = a._replace(hw=b.hw), b._replace(hw=a.hw)
    ref2 = sc.reference(a2, b2, _sd())
    moved = float(np.abs(ref2[2] - ref[2])[ref[2] > -20].max())
    print(f"reference |dZ| between the two arrangements: {moved:.2e}")
    assert moved > Z_ATOL, "vacuous: exchanging the image sizes does not move the reference"
    _compare("128x129", sc.run_gpu([a, b], [(0, 1)], _weights()), 0, ref)
    _compare("128x129 sizes exchanged", sc.run_gpu([a2, b2], [(0, 1)], _weights()), 0, ref2)


def test_shared_images():
    """Four images (200, 130, 64, 257 keypoints; three sizes), pairs (0,1) (1,2) (2,0) (1,0) (3,1) in one call: each
    against the reference, and each bit for bit what the pair gives alone at the same kmax."""
    imgs, refs = _shared()
    run = sc.run_gpu(imgs, sc.SHARED_PAIRS, _weights())
    assert run.kmax == 320
    for q, p in enumerate(sc.SHARED_PAIRS):
        _compare(f"shared {p}", run, q, refs[q])
    for q, p in enumerate(sc.SHARED_PAIRS):
        _same(run, sc.run_gpu(imgs, [p], _weights(), kmax=run.kmax), q)


def test_two_pass_dispatch_and_heavy_padding():
    """(2112, 2050) gives kmax 2112, the smallest above kSkFusedMaxK: the production dispatch takes sk_rows_kernel /
    sk_cols_kernel with no environment hook. Every 32nd row of Z plus the dustbin row, scores and matches against the
    float64 restatement (about 5 s on the CPU). A (150, 170) pair rides in the same call with 1,900 padding rows a
    side: its full Z."""
    big = sc.make_pair(*sc.BIG_SHAPE)
    small = sc.make_pair(*sc.BIG_PAD_SHAPE)
    run = sc.run_gpu([*big, *small], [(0, 1), (2, 3)], _weights())
    assert run.kmax == 2112
    n0 = sc.BIG_SHAPE[0]
    rows = np.concatenate([np.arange(0, n0, 32), [n0]])
    _compare("2112x2050", run, 0, sc.reference(*big, _sd()), rows=rows)
    _compare("150x170 at kmax 2112", run, 1, sc.reference(*small, _sd()))


@pytest.mark.parametrize("thr", [0.0, 0.2, 0.9])
@pytest.mark.parametrize("it", [0, 1, 20])
@pytest.mark.parametrize("nl", [2, 18])
def test_parameters(nl, it, thr):
    """(65, 127) with n_layers in {2, 18} (the packed blob holds that many layers of the same state dict),
    sinkhorn_iters in {0, 1, 20} (0 skips both loops: Z is the couplings minus the norm) and match_threshold in
    {0, 0.2, 0.9}, against the reference with the same parameters."""
    a, b, _ = _table_ref(65, 127)
    ref = sc.reference(a, b, _sd(), n_layers=nl, sinkhorn_iterations=it, match_threshold=thr)
    run = sc.run_gpu([a, b], [(0, 1)], _weights(nl), n_layers=nl, sinkhorn_iters=it, match_threshold=thr)
    _compare(f"65x127 layers {nl} iters {it} threshold {thr}", run, 0, ref, thr=thr)


def _raw_call(kmax_arg, n_pairs, ws_bytes_short=0, kmax_alloc=128):
    """gtsfm_superglue_batched called directly with sentinel-filled outputs; returns (rc, outputs unchanged?)."""
    from gtsfm_amd import native

    L = native.lib()
    a, b, _ = _table_ref(15, 17)
    kp, s, de, cnt, hw = sc.pack([a, b], kmax_alloc)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    kp, s, de, cnt, hw, pairs = t(kp), t(s), t(de), t(cnt), t(hw), t(np.array([[0, 1]], np.int32))
    need = L.gtsfm_superglue_workspace_bytes(1, kmax_alloc)
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
    idx = torch.full((1, kmax_alloc, 2), -7, dtype=torch.int32, device="cuda")
    c = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    ms = torch.full((1, kmax_alloc), -7.0, dtype=torch.float32, device="cuda")
    rc = L.gtsfm_superglue_batched(kp.data_ptr(), s.data_ptr(), de.data_ptr(), cnt.data_ptr(), hw.data_ptr(), 2,
                                   kmax_arg, pairs.data_ptr(), n_pairs, _weights().data_ptr(), 18, 20, 0.2,
                                   ws.data_ptr(), need - ws_bytes_short, idx.data_ptr(), c.data_ptr(), ms.data_ptr(),
                                   native.stream_handle())
    torch.cuda.synchronize()
    untouched = bool((ws == 0x5A).all() and (idx == -7).all() and (c == -7).all() and (ms == -7.0).all())
    return rc, untouched


def test_entry_point_checks():
    """kmax no multiple of 64 is GTSFM_ERR_ARG, a workspace one byte short GTSFM_ERR_CAPACITY, no pairs GTSFM_OK; none
    of the three launches anything (outputs and workspace keep their sentinels). The same call with nothing wrong
    returns GTSFM_OK and writes. The Python wrapper rejects the bad kmax before the library sees it."""
    from gtsfm_amd import device, native

    assert _raw_call(100, 1) == (native.GTSFM_ERR_ARG, True)
    assert _raw_call(128, 1, ws_bytes_short=1) == (native.GTSFM_ERR_CAPACITY, True)
    assert _raw_call(128, 0) == (native.GTSFM_OK, True)
    assert _raw_call(128, 1) == (native.GTSFM_OK, False)
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device="cuda")  # noqa: E731
    with pytest.raises(AssertionError, match="multiple of 64"):
        device.superglue_match(z(2, 100, 2), z(2, 100), z(2, 100, 256), z(2, dt=torch.int32), z(2, 2, dt=torch.int32),
                               z(1, 2, dt=torch.int32), _weights())
    idx, c, ms = device.superglue_match(z(2, 64, 2), z(2, 64), z(2, 64, 256), z(2, dt=torch.int32),
                                        z(2, 2, dt=torch.int32), z(0, 2, dt=torch.int32), _weights())
    assert idx.shape == (0, 64, 2) and c.shape == (0,) and ms.shape == (0, 64)


def test_zero_count_side():
    """A pair with an empty side handed straight to device.superglue_match (SuperGlueMatcher.match_batch filters such
    pairs on the host; the entry point does not need to). With m = 0 or n = 0 every index in sk_init_kernel,
    sk_pass_kernel, sk_vmerge_kernel, assign_rowmax_kernel, assign_colmax_kernel and sg_emit_kernel stays inside rows
    0..m and columns 0..n of the pair's (kmax + 1)^2 block: the score GEMM and the argmax loops run no iteration, the dustbin
    row / column is the only one read, and sg_emit_kernel reads idx0 / idx1 only when i < m and n > 0. (sk_norm(0, 0)
    is +inf, so a pair empty on both sides would carry NaN in u and v, which index nothing.) The empty pairs give
    count 0 and zero scores, and the pair beside them is bit for bit what it is alone."""
    imgs = sc.make_images([130, 64, 0], sc.SHARED_HW[:3], 43)
    pairs = [(0, 1), (0, 2), (2, 0)]
    run = sc.run_gpu(imgs, pairs, _weights(), kmax=192)
    for q in (1, 2):
        assert len(run.pairs_out[q]) == 0 and (run.mscores0[q] == 0).all()
    assert run.Z[1].shape == (131, 1) and run.Z[2].shape == (1, 131)
    _same(run, sc.run_gpu(imgs, [(0, 1)], _weights(), kmax=192), 0)
    _compare("130x64 beside empty pairs", run, 0, sc.reference(imgs[0], imgs[1], _sd()))


def test_chunked_equals_unchunked():
    """superglue_pairs_batched over the shared-image set, 1 and 2 pairs per launch sequence against all in one: the
    same dict, and the matches test_shared_images' single call emits. The features are 257 rows wide, so the
    generator's padding to a multiple of 64 runs too."""
    from gtsfm_amd.common.keypoints import Keypoints
    from gtsfm_amd.frontend.correspondence_generator.det_desc_correspondence_generator import (
        DeviceFeatures, superglue_pairs_batched)
    from gtsfm_amd.frontend.matcher.superglue_matcher import SuperGlueMatcher

    imgs, _ = _shared()
    kp, s, de, cnt, _ = sc.pack(imgs, max(sc.SHARED_COUNTS))
    t = lambda x: torch.from_numpy(x).cuda()  # noqa: E731
    feats = DeviceFeatures(t(kp), t(de), t(cnt), [Keypoints(i.kp, responses=i.scores) for i in imgs])
    feats.scores = t(s)
    matcher = SuperGlueMatcher(state_dict=_sd())
    shapes = [(*i.hw, 1) for i in imgs]
    whole = superglue_pairs_batched(matcher, feats, shapes, sc.SHARED_PAIRS)
    one = sc.run_gpu(imgs, sc.SHARED_PAIRS, _weights(), want_Z=False)
    assert list(whole) == list(sc.SHARED_PAIRS)
    print("matches per pair:", [len(v) for v in whole.values()])
    for q, p in enumerate(sc.SHARED_PAIRS):
        assert whole[p].dtype == np.uint32 and len(whole[p]) >= 5
        np.testing.assert_array_equal(whole[p], one.pairs_out[q])
    for chunk in (1, 2):
        got = superglue_pairs_batched(matcher, feats, shapes, sc.SHARED_PAIRS, chunk=chunk)
        assert list(got) == list(whole)
        for p in whole:
            np.testing.assert_array_equal(got[p], whole[p])
