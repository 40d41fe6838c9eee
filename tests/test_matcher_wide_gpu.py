"""GTSFM_MATCH_F16_RERANK for descriptors of 257..512 dimensions (D2-Net's 512-D): the 32-row-chunk shortlist kernel.

Bar, as for the 256-D suite: the matches (indices and their order) are identical to GTSFM_MATCH_EXACT_F32 on every
pair and to the oracle's TwoWayMatcher restatement (oracle/twoway.c) on the first pairs. Shapes are the smallest that
reach every path: the first column past the old 256 pad, dims that are no multiple of 16 or of 4, counts around the
shortlist size (8), the chunk height (32) and the query block (128), a kmax that is no multiple of 128, ties, values
outside the fp16 range, and clustered descriptors whose (pair, side)s go whole to the exact tile kernel.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DIM = 512


@pytest.fixture(scope="module")
def dev():
    from gtsfm_amd import native

    native.require_gpu()
    native.lib()
    return torch.device("cuda")


def unit(rng, n, dim):
    x = rng.normal(size=(n, dim))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def planted(rng, n1, n2, dim=DIM, frac=0.3, noise=0.15):
    """Two sets of random unit vectors; a share `frac` of the second are noisy copies of rows of the first."""
    a, b = unit(rng, n1, dim), unit(rng, n2, dim)
    k = int(frac * min(n1, n2))
    src, dst = rng.permutation(n1)[:k], rng.permutation(n2)[:k]
    y = a[src] + noise * rng.normal(size=(k, dim)) / np.sqrt(dim)
    b[dst] = (y / np.linalg.norm(y, axis=1, keepdims=True)).astype(np.float32)
    return a, b


def clustered(rng, centres, n):
    """Rows 3e-3 away from one of a few centres: distances within a cluster agree far below the fp16 error bound."""
    dim = centres.shape[1]
    return (centres[rng.integers(0, len(centres), n)] + 3e-3 * rng.normal(size=(n, dim)) / np.sqrt(dim)).astype(
        np.float32)


def stats_batch():
    """The inputs of test_rerank_stats_512 (also what the CPU emulation quoted in its docstring ran on)."""
    rng = np.random.default_rng(512077)
    centres = unit(rng, 4, DIM)
    descs = [clustered(rng, centres, 700), clustered(rng, centres, 1000)]
    descs += list(planted(rng, 900, 650))
    return descs


def upload(dev, descs):
    kmax = max(len(d) for d in descs)
    arr = np.zeros((len(descs), kmax, descs[0].shape[1]), np.float32)
    for i, d in enumerate(descs):
        arr[i, : len(d)] = d
    return torch.from_numpy(arr).to(dev), torch.tensor([len(d) for d in descs], dtype=torch.int32, device=dev)


def run(dev, descs, pairs, ratio, mode):
    from gtsfm_amd import device

    desc_t, cnt = upload(dev, descs)
    idx, m = device.match_pairs(desc_t, cnt, torch.tensor(pairs, dtype=torch.int32, device=dev), ratio, mode)
    m = m.cpu().numpy()
    idx = idx.cpu().numpy().view(np.uint32)
    return [idx[p, : m[p]].copy() for p in range(len(pairs))]


def check(dev, oracle_mod, descs, pairs, ratio, n_oracle=2):
    from gtsfm_amd import native

    fast = run(dev, descs, pairs, ratio, native.GTSFM_MATCH_F16_RERANK)
    exact = run(dev, descs, pairs, ratio, native.GTSFM_MATCH_EXACT_F32)
    for p, (f, e) in enumerate(zip(fast, exact)):
        np.testing.assert_array_equal(f, e, err_msg=f"pair {pairs[p]}")
    for p in range(min(n_oracle, len(pairs))):
        i1, i2 = pairs[p]
        if len(descs[i1]) == 0 or len(descs[i2]) == 0:
            assert fast[p].size == 0, f"pair {pairs[p]} has an empty side"
            continue
        ref = oracle_mod.twoway_match(descs[i1], descs[i2], ratio).reshape(-1, 2)
        np.testing.assert_array_equal(fast[p].reshape(-1, 2), ref, err_msg=f"oracle pair {pairs[p]}")
    return fast


@pytest.mark.parametrize("ratio", [0.8, None])
@pytest.mark.parametrize("dim", [257, 384, 500, 511, 512, 513, 600])
def test_dims(dev, oracle_mod, dim, ratio):
    """257: first column past the 256 pad (255 zero columns); 500: no multiple of 16; 511: the re-rank's scalar
    (non-float4) row walk; 513 and 600: past the shortlist kernel's width, through the exact kernels."""
    rng = np.random.default_rng(dim)
    a, b = planted(rng, 500, 600, dim)
    out = check(dev, oracle_mod, [a, b], [(0, 1), (1, 0)], ratio)
    assert len(out[0]) > 50  # the planted matches are found


@pytest.mark.parametrize("ratio", [0.8, None])
def test_ragged_counts_one_batch(dev, oracle_mod, ratio):
    """Counts 0, 1, 7, 8 (at or below the shortlist size), 33 (one past the 32-row chunk), 129 and 257 (one past a
    128-query block), and 777 / 1000 / 1200 in one batch with kmax = 1200 (no multiple of 128); pairs in both orders
    and images paired with themselves."""
    rng = np.random.default_rng(33)
    sizes = [1000, 33, 129, 257, 8, 7, 1, 0, 777, 1200]
    base = unit(rng, 1200, DIM)
    descs = []
    for s in sizes:  # views share a latent set: planted matches between every pair
        d = unit(rng, s, DIM)
        k = s // 3
        if k:
            y = base[rng.permutation(1200)[:k]] + 0.15 * rng.normal(size=(k, DIM)) / np.sqrt(DIM)
            d[rng.permutation(s)[:k]] = y / np.linalg.norm(y, axis=1, keepdims=True)
        descs.append(d.astype(np.float32))
    pairs = [(0, 1), (1, 0), (2, 3), (4, 0), (0, 4), (5, 9), (6, 0), (0, 6), (1, 1), (8, 8)]
    for big in (0, 9):  # every image against the two largest, in both orders
        for i in range(len(sizes)):
            pairs += [q for q in ((i, big), (big, i)) if q not in pairs]
    out = check(dev, oracle_mod, descs, pairs, ratio, n_oracle=10)
    assert len(out[pairs.index((0, 9))]) > 50
    assert all(out[p].size == 0 for p, (i, j) in enumerate(pairs) if 7 in (i, j))
    for p in (8, 9):  # an image against itself: every keypoint is its own mutual nearest neighbour, at distance 0
        n = sizes[pairs[p][0]]
        if ratio is None:
            assert np.array_equal(out[p].reshape(-1, 2), np.stack([np.arange(n)] * 2, 1))


@pytest.mark.parametrize("ratio", [0.8, None])
def test_ties_and_duplicate_rows(dev, oracle_mod, ratio):
    rng = np.random.default_rng(3)
    a, b = planted(rng, 400, 400)
    b[10:20] = a[50:60]  # exact copies
    b[20:30] = a[50:60]  # ... twice: tied nearest neighbours
    a[100:105] = a[0]  # duplicate query rows
    b[200] = b[201]
    check(dev, oracle_mod, [a, b], [(0, 1), (1, 0)], ratio)


def test_values_outside_fp16_range(dev, oracle_mod):
    """An image with one value above 60000 and one with an inf are flagged unsafe: every pair that touches them is
    recomputed exactly, the others keep the shortlist."""
    rng = np.random.default_rng(5)
    a, b = planted(rng, 300, 350)
    c, d = planted(rng, 200, 260)
    big = b.copy()
    big[17, 400] = 7.0e4
    inf = d.copy()
    inf[5, 511] = np.inf
    descs = [a, big, c, inf, b]
    for ratio in (0.8, None):
        check(dev, oracle_mod, descs, [(0, 1), (2, 3), (3, 0), (1, 2), (0, 4)], ratio, n_oracle=3)


def test_clustered_pairs_use_exact_tiles(dev, oracle_mod):
    """Clustered pairs (most shortlists uncertified: the whole (pair, side) goes to fl_exact_tile_kernel) mixed with
    planted pairs (few uncertified: per-keypoint rescans) and ragged counts in one batch."""
    rng = np.random.default_rng(60 + DIM)
    centres = unit(rng, 4, DIM)
    a, b = clustered(rng, centres, 700), clustered(rng, centres, 1000)
    c, d = planted(rng, 900, 650)
    descs = [a, b, c, d, clustered(rng, centres, 65)]
    pairs = [(0, 1), (2, 3), (1, 0), (0, 3), (4, 1), (3, 4)]
    for ratio in (0.8, None):
        check(dev, oracle_mod, descs, pairs, ratio, n_oracle=3)


def test_rerank_stats_512(dev):
    """device.match_pairs(..., stats=) at 512-D: clustered pairs go whole to the exact tiles, planted ones certify
    nearly everything, and the per-side counts add up.

    The 0.05 cap on the planted pair is a condition on the inputs. A numpy emulation of the shortlist keys (operands
    rounded to fp16, products summed exactly, |b|^2 - 2 a.b in fp32) and of fl_rerank_kernel's key_eps on
    stats_batch()'s planted pair leaves 0 of its 1550 (keypoint, side)s without the certificate (mean key_eps 3.2e-3;
    the gap between the 2nd and the 8th of 650 random unit rows is ~4e-2), so the reference arithmetic alone stays far
    below the cap at noise 0.15; both sides of the clustered pair come out wholly uncertified, as the test expects."""
    from gtsfm_amd import device, native

    descs = stats_batch()
    desc_t, cnt = upload(dev, descs)
    for pairs, clustered_sides in (([(2, 3)], 0), ([(0, 1), (2, 3)], 1700)):
        st = {}
        device.match_pairs(desc_t, cnt, torch.tensor(pairs, dtype=torch.int32, device=dev), 0.8,
                           native.GTSFM_MATCH_F16_RERANK, stats=st)
        sides = sum(len(descs[i]) + len(descs[j]) for i, j in pairs)
        assert st["keypoint_sides"] == sides
        assert 0 <= st["rescan_frac"] <= st["uncertified_frac"] <= 1 and 0 <= st["tiled_frac"] <= 1
        assert st["uncertified"] == round(st["uncertified_frac"] * sides)
        # every uncertified entry is either in a tiled (pair, side) or rescanned on its own
        assert st["uncertified_frac"] <= st["tiled_frac"] + st["rescan_frac"] + 1e-12
        assert abs(st["tiled_frac"] - clustered_sides / sides) < 1e-9
        if clustered_sides == 0:  # no tiled side: the per-side counts are the rescans and sum to the total
            assert round(st["rescan_frac"] * sides) == st["uncertified"]
            assert st["uncertified_frac"] < 0.05
    st = {}
    device.match_pairs(desc_t, cnt, torch.tensor([(2, 3)], dtype=torch.int32, device=dev), 0.8,
                       native.GTSFM_MATCH_EXACT_F32, stats=st)
    assert st == {}


def test_twoway_matcher_512d_uses_rerank(dev, oracle_mod, monkeypatch):
    """The per-call plugin on D2-Net-sized descriptors with NaN rows: the oracle's matches (indices of the unfiltered
    arrays), and the mode handed to device.match_pairs is F16_RERANK."""
    from gtsfm_amd import device, native
    from gtsfm_amd.frontend.matcher.twoway_matcher import TwoWayMatcher

    rng = np.random.default_rng(8)
    a, b = planted(rng, 300, 340)
    a[[3, 150]] = np.nan
    b[77, 9] = np.nan
    modes = []
    real = device.match_pairs

    def spy(desc, counts, pairs, ratio, mode, *args, **kwargs):
        modes.append(mode)
        return real(desc, counts, pairs, ratio, mode, *args, **kwargs)

    monkeypatch.setattr(device, "match_pairs", spy)
    got = TwoWayMatcher(ratio_test_threshold=0.8).match(None, None, a, b, (480, 640, 3), (480, 640, 3))
    assert modes == [native.GTSFM_MATCH_F16_RERANK]
    va = np.nonzero(~np.isnan(a).any(axis=1))[0]
    vb = np.nonzero(~np.isnan(b).any(axis=1))[0]
    ref = oracle_mod.twoway_match(a[va], b[vb], 0.8).reshape(-1, 2)
    assert len(ref) > 30
    np.testing.assert_array_equal(got, np.stack([va[ref[:, 0]], vb[ref[:, 1]]], 1))
