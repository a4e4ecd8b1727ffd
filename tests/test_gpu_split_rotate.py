"""The head of a split-kernel tile (csrc/wagg_dense_split.inc: the W split, two instructions a low-part pair, and the
first fragment reads): k-slices of 0 to 4 tiles -- none, a single tile, the ring's prologue and its last tiles -- for every
instantiated row-block count MT, the split form against the exact fp32 kernel within the split form's documented bound and
against the fp64 oracle; and NaN, +-inf and all-zero columns in the first and in the last tile of a slice, the tiles that
the prologue and the clamped re-loads of the last tiles handle."""
import numpy as np
import pytest

from tests.test_gpu_dense_split import _bound, _maxrel

pytestmark = pytest.mark.gpu

KSPLIT = 8
# G -> k tiles of 32 cells over 8 slices: 5 (1 tile each, three slices empty), 8 (1 each), 16 (2), 24 (3), 32 (4); 1000 has a
# partial last tile (32 tiles, 4 each)
GS = [160, 256, 512, 768, 1024, 1000]
MTS = [1, 2, 3, 4, 5, 6, 8, 10, 12, 14, 16, 18, 20, 21, 22, 23]
T_OF_MT = {m: 16 * m - (m % 5) for m in MTS}            # one row block of MT x 16 rows, the last one partly filled


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch


def _slice_tiles(G):
    """(first cell of the first tile, first cell of the last tile) of every non-empty k-slice."""
    n_kt = (G + 31) // 32
    kps = (n_kt + KSPLIT - 1) // KSPLIT
    out = []
    for s in range(KSPLIT):
        k0, k1 = s * kps, min((s + 1) * kps, n_kt)
        if k1 > k0:
            out.append((32 * k0, 32 * (k1 - 1)))
    return out


def _apply_both(plan, X, torch):
    Xd = torch.from_numpy(X).cuda()
    return (plan.apply(Xd, ksplit=KSPLIT).cpu().numpy(), plan.apply(Xd, ksplit=KSPLIT, exact=True).cpu().numpy())


@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("MT", MTS)
def test_every_mt_every_slice_length(torch_cuda, MT, G):
    from climate_toolbox_amd.engine import DensePlan
    from oracle import ref_numpy as O
    T, R = T_OF_MT[MT], 270                                 # two column tiles, the second partly filled
    rng = np.random.default_rng(MT * 10000 + G)
    W = rng.uniform(0, 1, (G, R)).astype(np.float32)
    X = (280 + 30 * rng.standard_normal((T, G))).astype(np.float32)
    plan = DensePlan.from_host(W)
    ref = O.agg_dense(X, W)
    got, ex = _apply_both(plan, X, torch_cuda)
    bound = _bound(X, W)
    e_split, e_exact = _maxrel(got, ref), _maxrel(ex, ref)
    print("MT=%d G=%d: split %.3g, exact %.3g, |split - exact| / bound %.3g" % (
        MT, G, e_split, e_exact, float(np.max(np.abs(got.astype(np.float64) - ex) / bound))))
    assert np.all(np.abs(got.astype(np.float64) - ex) <= bound)
    assert np.all(np.abs(got - ref) <= bound)
    assert e_split <= max(2 * e_exact, 2e-6)


@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("T", [40, 365])
def test_special_values_in_first_and_last_tiles(torch_cuda, T, G):
    from climate_toolbox_amd.engine import DensePlan
    from oracle import ref_numpy as O
    torch = torch_cuda
    rng = np.random.default_rng(T + G)
    R = 270
    tiles = _slice_tiles(G)
    first0, last0 = tiles[0]                                # the first slice
    firstn, lastn = tiles[-1]                               # the last non-empty slice
    edge = sorted({first0, last0, firstn, lastn})
    W = rng.uniform(0, 1, (G, R)).astype(np.float32)
    W[:, 5] = 0.0                                           # all-zero columns: 0 / 0 stays NaN, in both column tiles
    W[:, 260] = 0.0
    for c, k in zip((7, 9, 261, 263), (first0, last0, firstn, lastn)):
        W[k:k + 32, c] = 0.0                                # a column that is zero in one edge tile only
    X = (rng.standard_normal((T, G)) * 100).astype(np.float32)
    X[4, :] = np.nan                                        # an all-NaN row: result 0
    for i, k in enumerate(edge):
        X[2, k:k + 32:3] = np.nan                           # NaN -> 0 in every edge tile
        X[6 + i, k:k + 32] = np.nan                         # a row with one whole edge tile of NaN
    plan = DensePlan.from_host(W)
    ref = O.agg_dense(X, W)
    got, ex = _apply_both(plan, X, torch)
    fin = np.isfinite(ref)
    bound = _bound(X, W)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    np.testing.assert_array_equal(np.isnan(ex), np.isnan(ref))
    assert np.isnan(got[:, 5]).all() and np.isnan(got[:, 260]).all()
    assert np.all(np.abs(got - ref)[fin] <= bound[fin])
    assert np.all(np.abs(got.astype(np.float64) - ex)[fin] <= bound[fin])
    np.testing.assert_array_equal(got[4][~np.isnan(got[4])], 0.0)
    assert not plan.saw_inf()
    # +-inf in the edge tiles: the caller is told, the rows that hold one are not finite wherever the cell has weight, and
    # every other row keeps its bits (rows do not mix)
    Xi = X.copy()
    rows = {}
    for i, k in enumerate(edge):
        r = 12 + i
        g = min(k + 1 + 7 * i, G - 1)
        Xi[r, g] = np.inf if i % 2 == 0 else -np.inf
        rows[r] = g
    goti = plan.apply(torch.from_numpy(Xi).cuda(), ksplit=KSPLIT).cpu().numpy()
    assert plan.saw_inf()
    clean = np.array([t not in rows for t in range(T)])
    np.testing.assert_array_equal(goti[clean], got[clean])
    for r, g in rows.items():
        assert not np.isfinite(goti[r][W[g] > 0]).any(), (r, g)
