"""The split kernel's pipeline (csrc/wagg_dense_split.inc: W straight to registers, a ring of three X tiles in LDS): k-slices
of 0, 1, 2 and 3 tiles (the ring's prologue and epilogue), every instantiated row-block count MT, special values and the
transforms, each against the C oracle within the split form's documented bound and against the exact fp32 kernel."""
import numpy as np
import pytest

from tests.test_gpu_dense_split import _bound, _maxrel

pytestmark = pytest.mark.gpu

KSPLIT = 8
# G -> k tiles of 32 cells: 5 (slices of 1 tile, three slices empty), 8 (1 each), 16 (2 each), 24 (3 each); 500 has a
# partial last tile
GS = [160, 256, 512, 768, 500]
# one T per instantiated MT (T <= 368: one row block of MT x 16 rows, MT the smallest of the set with 16 MT >= T)
MTS = [1, 2, 3, 4, 5, 6, 8, 10, 12, 14, 16, 18, 20, 21, 22, 23]
T_OF_MT = {m: 16 * m - (m % 5) for m in MTS}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch


def _synth_w(G, R, seed):
    """The synthetic weights of DensePlan.synth over their column sums, from the C oracle (identity rows of X pick them
    out): the split form's bound does not change when a column is scaled."""
    from oracle import c_oracle
    return c_oracle.dense_synth(np.eye(G, dtype=np.float32), 0, G, R, 0, R, seed).astype(np.float32)


def _check(plan, X, W, ref, torch, **kw):
    Xd = torch.from_numpy(X).cuda()
    got = plan.apply(Xd, ksplit=KSPLIT, **kw).cpu().numpy()
    ex = plan.apply(Xd, ksplit=KSPLIT, exact=True, **kw).cpu().numpy()
    fin = np.isfinite(ref)
    bound = _bound(X, W)
    assert np.all(np.abs(got - ref)[fin] <= bound[fin])
    assert np.all(np.abs(ex - ref)[fin] <= bound[fin])
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    return got, ex


@pytest.mark.parametrize("G", GS)
def test_short_slices(torch_cuda, G):
    """k-slices of 0-3 tiles, T = 365 (MT = 23): the C oracle and the exact kernel; the default k split gives the same
    result up to the order of the slice sums."""
    from climate_toolbox_amd.engine import DensePlan
    from oracle import c_oracle
    R, seed, T = 300, 13, 365
    plan = DensePlan.synth(G, R, seed)
    rng = np.random.default_rng(G)
    X = (280 + 30 * rng.standard_normal((T, G))).astype(np.float32)
    ref = c_oracle.dense_synth(X, 0, G, R, 0, R, seed)
    got, ex = _check(plan, X, _synth_w(G, R, seed), ref, torch_cuda)
    print("G=%d: split %.3g, exact %.3g" % (G, _maxrel(got, ref), _maxrel(ex, ref)))
    assert _maxrel(got, ref) <= max(2 * _maxrel(ex, ref), 2e-6)


@pytest.mark.parametrize("MT", MTS)
def test_every_mt(torch_cuda, MT):
    """One T per instantiated MT, slices of 3 tiles (G = 768) and of 1 tile with empty slices (G = 160)."""
    from climate_toolbox_amd.engine import DensePlan
    from oracle import c_oracle
    T, R, seed = T_OF_MT[MT], 260, 7 + MT
    for G in (768, 160):
        plan = DensePlan.synth(G, R, seed)
        rng = np.random.default_rng(MT * 1000 + G)
        X = (280 + 30 * rng.standard_normal((T, G))).astype(np.float32)
        ref = c_oracle.dense_synth(X, 0, G, R, 0, R, seed)
        got, ex = _check(plan, X, _synth_w(G, R, seed), ref, torch_cuda)
        assert _maxrel(got, ref) <= max(2 * _maxrel(ex, ref), 2e-6), (MT, G)


@pytest.mark.parametrize("G", [160, 512, 768])
def test_nan_inf_zero_columns(torch_cuda, G):
    from climate_toolbox_amd.engine import DensePlan
    from oracle import ref_numpy as O
    torch = torch_cuda
    rng = np.random.default_rng(G + 1)
    R, T = 270, 40
    W = rng.uniform(0, 1, (G, R)).astype(np.float32)
    W[:, 5] = 0.0                                           # all-zero column: 0 / 0 stays NaN
    W[:, 260] = 0.0                                         # ... in the second column tile too
    X = (rng.standard_normal((T, G)) * 100).astype(np.float32)
    X[2, ::3] = np.nan                                      # NaN -> 0
    X[4, :] = np.nan                                        # an all-NaN row: result 0
    X[:, 40:72] = np.nan                                    # a whole k tile of NaN
    plan = DensePlan.from_host(W)
    ref = O.agg_dense(X, W)
    got, ex = _check(plan, X, W, ref, torch)
    assert np.isnan(got[:, 5]).all() and np.isnan(got[:, 260]).all()
    np.testing.assert_array_equal(got[4][~np.isnan(got[4])], 0.0)
    assert not plan.saw_inf()
    Xi = X.copy()
    Xi[7, G - 1] = np.inf                                   # in the last tile of the last non-empty slice
    Xi[8, 0] = -np.inf
    plan.apply(torch.from_numpy(Xi).cuda(), ksplit=KSPLIT)
    assert plan.saw_inf()


@pytest.mark.parametrize("G", [160, 512, 768])
def test_poly_and_edd(torch_cuda, G):
    from climate_toolbox_amd.engine import DensePlan
    from oracle import ref_numpy as O
    torch = torch_cuda
    rng = np.random.default_rng(G + 2)
    R, T = 140, 33
    W = rng.uniform(0, 1, (G, R)).astype(np.float32)
    tmin = (10 + 8 * rng.standard_normal((T, G))).astype(np.float32)
    tmax = tmin + np.abs(6 * rng.standard_normal((T, G))).astype(np.float32)
    plan = DensePlan.from_host(W)
    Xd, X2d = torch.from_numpy(tmin).cuda(), torch.from_numpy(tmax).cuda()
    for power in (1, 2, 3):
        Xp = (tmin.astype(np.float64) + 1.5) ** power
        ref = O.agg_dense(Xp, W)
        got = plan.apply_poly(Xd, 1.5, power, ksplit=KSPLIT).cpu().numpy()
        ex = plan.apply_poly(Xd, 1.5, power, ksplit=KSPLIT, exact=True).cpu().numpy()
        bound = _bound(Xp.astype(np.float32), W) + 2e-6 * np.abs(ref)   # + the transform's own fp32 rounding
        assert np.all(np.abs(got - ref) <= bound), power
        assert np.all(np.abs(ex - ref) <= bound), power
    got = plan.apply_edd(Xd, X2d, 12.0, ksplit=KSPLIT).cpu().numpy()
    ex = plan.apply_edd(Xd, X2d, 12.0, ksplit=KSPLIT, exact=True).cpu().numpy()
    # the exact kernel on the same transformed field is the reference for the transform; the split adds its bound
    assert np.all(np.abs(got - ex) <= 4e-6 * np.abs(ex) + 1e-6 * np.abs(ex).max())
