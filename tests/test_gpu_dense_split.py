"""Split form of fp32 full-form dense plans (f16 high + low parts of both operands on the f16 matrix pipe,
csrc/wagg_dense_split.inc): accuracy against the fp64 oracle and the exact fp32 kernel (``exact=True``), the
documented error bound, special values, transforms, and the column scales of every builder."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch


def _maxrel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    return float(np.max(np.abs(got[fin] - ref[fin]) / np.maximum(np.abs(ref[fin]), 1e-30))) if fin.any() else 0.0


def _bound(X, W):
    """The documented bound of the split form (dense section), per (t, r): 4e-6 of sum |x| |w| / den (three
    products of 22-bit parts, the dropped xl.wl, the fp32 sums) plus the absolute floor of subnormal low parts: 2^-36 of
    the row maximum and 2^-36 of the column maximum times sum |x| / den."""
    Xz = np.where(np.isnan(X), 0.0, X).astype(np.float64)
    W = W.astype(np.float64)
    den = W.sum(0)[None, :]
    ax, aw = np.abs(Xz), np.abs(W)
    xmax = ax.max(1, keepdims=True)
    wmax = aw.max(0, keepdims=True)
    return (4e-6 * (ax @ aw) + 2.0 ** -36 * xmax * aw.sum(0)[None, :] + 2.0 ** -36 * wmax * ax.sum(1, keepdims=True)) / np.abs(den)


def _both(plan, X, torch, **kw):
    Xd = torch.from_numpy(X).cuda()
    return plan.apply(Xd, **kw).cpu().numpy(), plan.apply(Xd, exact=True, **kw).cpu().numpy()


@pytest.mark.parametrize("T,G,R", [(40, 3000, 300), (37, 1000, 100), (365, 2048, 600), (1369, 640, 256), (5, 96, 7)])
def test_split_vs_exact_vs_oracle(torch_cuda, T, G, R):
    from climate_toolbox_amd.engine import DensePlan
    from oracle import ref_numpy as O
    rng = np.random.default_rng(T * G + R)
    W = rng.uniform(0, 1, (G, R)).astype(np.float32)
    X = (280 + 30 * rng.standard_normal((T, G))).astype(np.float32)
    ref = O.agg_dense(X, W)
    plan = DensePlan.from_host(W)
    got, ex = _both(plan, X, torch_cuda)
    e_split, e_exact = _maxrel(got, ref), _maxrel(ex, ref)
    print("T=%d G=%d R=%d: split %.3g, exact %.3g" % (T, G, R, e_split, e_exact))
    assert e_split <= max(2 * e_exact, 2e-6)
    assert np.all(np.abs(got - ref) <= _bound(X, W))
    # row blocks are independent: the first rows alone give the same bits
    np.testing.assert_array_equal(plan.apply(torch_cuda.from_numpy(X[: min(T, 24)]).cuda()).cpu().numpy(), got[: min(T, 24)])


def test_split_constant_field(torch_cuda):
    from climate_toolbox_amd.engine import DensePlan
    rng = np.random.default_rng(5)
    W = rng.uniform(0, 1, (4096, 300)).astype(np.float32)
    X = np.full((30, 4096), 273.15, np.float32)
    got, ex = _both(DensePlan.from_host(W), X, torch_cuda)
    ref = np.float64(np.float32(273.15))
    e_split, e_exact = np.max(np.abs(got / ref - 1)), np.max(np.abs(ex / ref - 1))
    print("constant field: split %.3g, exact %.3g" % (e_split, e_exact))
    assert e_split <= max(2 * e_exact, 2e-6)


@pytest.mark.parametrize("decades", [6, 9, 12])
def test_split_dynamic_range_rows(torch_cuda, decades):
    from climate_toolbox_amd.engine import DensePlan
    from oracle import ref_numpy as O
    rng = np.random.default_rng(decades)
    G, R = 2000, 200
    W = rng.uniform(0, 1, (G, R)).astype(np.float32)
    X = (10.0 ** rng.uniform(-decades, 0, (20, G)) * rng.choice([-1.0, 1.0], (20, G))).astype(np.float32)
    X[3] *= 1e20
    X[4] *= 1e-20
    got, ex = _both(DensePlan.from_host(W), X, torch_cuda)
    ref = O.agg_dense(X, W)
    assert np.all(np.abs(got - ref) <= _bound(X, W))
    assert np.all(np.abs(ex - ref) <= _bound(X, W))


def test_split_extreme_and_lognormal_columns(torch_cuda):
    from climate_toolbox_amd.engine import DensePlan
    from oracle import ref_numpy as O
    rng = np.random.default_rng(11)
    G, R = 1000, 96
    W = rng.uniform(0, 1, (G, R))
    W[:, 0:8] *= 1e-30
    W[:, 8:16] *= 1e30
    W[:, 16:48] = rng.lognormal(0, 2, (G, 32))          # popwt-like: a few cells carry most of the weight
    W[::7, 48:56] = 0.0
    W = W.astype(np.float32)
    X = (280 + 30 * rng.standard_normal((25, G))).astype(np.float32)
    ref = O.agg_dense(X, W)
    got, ex = _both(DensePlan.from_host(W), X, torch_cuda)
    e_split, e_exact = _maxrel(got, ref), _maxrel(ex, ref)
    print("extreme columns: split %.3g, exact %.3g" % (e_split, e_exact))
    assert e_split <= max(2 * e_exact, 2e-6)
    assert np.all(np.abs(got - ref) <= _bound(X, W))


def test_split_nan_inf_and_zero_columns(torch_cuda):
    from climate_toolbox_amd.engine import DensePlan
    from oracle import ref_numpy as O
    torch = torch_cuda
    rng = np.random.default_rng(3)
    G, R = 600, 80
    W = rng.uniform(0, 1, (G, R)).astype(np.float32)
    W[:, 5] = 0.0                                          # all-zero column: 0 / 0 stays NaN (S7)
    X = (rng.standard_normal((12, G)) * 100).astype(np.float32)
    X[2, ::3] = np.nan                                     # NaN -> 0 (S6)
    X[4, :] = np.nan                                       # an all-NaN row: scale 0, result 0
    plan = DensePlan.from_host(W)
    ref = O.agg_dense(X, W)
    got, ex = _both(plan, X, torch)
    assert np.isnan(got[:, 5]).all() and np.isnan(ex[:, 5]).all()
    assert not plan.saw_inf()
    # zero-mean data: the sums cancel, so relative errors say nothing; both forms keep the bound of sum |x| |w|
    fin = np.isfinite(ref)
    assert np.all(np.abs(got - ref)[fin] <= _bound(X, W)[fin])
    assert np.all(np.abs(ex - ref)[fin] <= _bound(X, W)[fin])
    np.testing.assert_array_equal(got[4][~np.isnan(got[4])], 0.0)
    Xi = X.copy()
    Xi[7, 10] = np.inf
    Xi[8, 11] = -np.inf
    plan.apply(torch.from_numpy(Xi).cuda())
    assert plan.saw_inf()
    plan.apply(torch.from_numpy(Xi).cuda(), exact=True)
    assert plan.saw_inf()


def test_split_poly_and_edd(torch_cuda):
    from climate_toolbox_amd.engine import DensePlan
    from oracle import ref_numpy as O
    torch = torch_cuda
    rng = np.random.default_rng(8)
    G, R, T = 1500, 120, 30
    W = rng.uniform(0, 1, (G, R)).astype(np.float32)
    tmin = (10 + 8 * rng.standard_normal((T, G))).astype(np.float32)
    tmax = tmin + np.abs(6 * rng.standard_normal((T, G))).astype(np.float32)
    plan = DensePlan.from_host(W)
    Xd, X2d = torch.from_numpy(tmin).cuda(), torch.from_numpy(tmax).cuda()
    for power in (1, 2, 4):
        ref = O.agg_dense((tmin.astype(np.float64) + 1.5) ** power, W)
        got = plan.apply_poly(Xd, 1.5, power).cpu().numpy()
        ex = plan.apply_poly(Xd, 1.5, power, exact=True).cpu().numpy()
        assert _maxrel(got, ref) <= max(2 * _maxrel(ex, ref), 2e-6), power
    got = plan.apply_edd(Xd, X2d, 12.0).cpu().numpy()
    ex = plan.apply_edd(Xd, X2d, 12.0, exact=True).cpu().numpy()
    # the exact kernel on the same transformed field is the reference for the transform; the split adds its bound
    assert np.all(np.abs(got - ex) <= 4e-6 * np.abs(ex) + 1e-6 * np.abs(ex).max())


def test_split_exact_flag_and_host_path(torch_cuda):
    from climate_toolbox_amd.engine import DensePlan
    torch = torch_cuda
    rng = np.random.default_rng(21)
    G, R, T = 2000, 300, 50
    W = rng.uniform(0, 1, (G, R)).astype(np.float32)
    X = (280 + 30 * rng.standard_normal((T, G))).astype(np.float32)
    plan = DensePlan.from_host(W)
    got, ex = _both(plan, X, torch)
    assert not np.array_equal(got, ex)                      # two different kernels ...
    np.testing.assert_array_equal(plan.apply(torch.from_numpy(X).cuda(), exact=True).cpu().numpy(), ex)   # ... each deterministic
    np.testing.assert_array_equal(plan.apply_host(X), got)
    np.testing.assert_array_equal(plan.apply_host(X, exact=True), ex)
    # scaling X by a power of two scales the result exactly, in either form
    np.testing.assert_array_equal(plan.apply(torch.from_numpy(2 * X).cuda()).cpu().numpy(), 2 * got)


def test_split_column_scales_same_for_every_builder(torch_cuda):
    """The column scales come from the stored W: plans of the same W from every builder (and a clone) give the same bits."""
    from climate_toolbox_amd.engine import DensePlan
    torch = torch_cuda
    rng = np.random.default_rng(4)
    G, R, T = 1200, 260, 20
    W = rng.uniform(0, 1, (G, R)).astype(np.float32)
    W[rng.uniform(size=(G, R)) < 0.5] = 0.0
    W[:, 7] *= 1e-12
    X = (280 + 30 * rng.standard_normal((T, G))).astype(np.float32)
    Xd = torch.from_numpy(X).cuda()
    host = DensePlan.from_host(W)
    base = host.apply(Xd).cpu().numpy()
    g, r = np.nonzero(W)
    rowptr = np.zeros(G + 1, np.int64)
    np.add.at(rowptr, g + 1, 1)
    rowptr = np.cumsum(rowptr)
    csr = DensePlan.from_csr(rowptr, r.astype(np.int32), W[g, r].astype(np.float64), G, R, form="full")
    seg = DensePlan.from_segments(g.astype(np.int32), r.astype(np.int32), W[g, r].astype(np.float64), G, R, form="full")
    for p in (csr, seg, host.replica(host.device)):
        assert p.info["form"] == 0
        got = p.apply(Xd).cpu().numpy()
        # denominators of the table builders are fp64 sums of the table (equal to the host plan's to the last bit here)
        np.testing.assert_array_equal(got, base)
    # synth: its own W, checked against the exact kernel on the same plan
    sp = DensePlan.synth(G, R, 9)
    s_got, s_ex = _both(sp, X, torch)
    assert np.max(np.abs(s_got - s_ex) / np.abs(s_ex)) < 4e-6
    assert np.max(np.abs(sp.replica(sp.device).apply(Xd).cpu().numpy() - s_got)) == 0.0


def test_split_accuracy_full_size(torch_cuda):
    """c2-dense size (101 GB W): one 16-column window in every column tile, all 1,036,800 cells, against the C oracle."""
    from climate_toolbox_amd import engine
    from oracle import c_oracle
    from tests.test_gpu_parity import _tile_windows
    G, R, seed = 720 * 1440, 24378, 2
    try:
        plan = engine.DensePlan.synth(G, R, seed)
    except Exception as e:                      # a box without 110 GB free HBM cannot hold the operand
        pytest.skip("dense W does not fit: %s" % e)
    X = engine.synth_field(24, G, seed=5, base=280.0, amp=60.0)
    got, ex = plan.apply(X).cpu().numpy(), plan.apply(X, exact=True).cpu().numpy()
    cols = _tile_windows(R, 16, seed=20)
    ref = c_oracle.dense_synth_cols(X.cpu().numpy(), G, R, cols, seed)
    e_split, e_exact = _maxrel(got[:, cols], ref), _maxrel(ex[:, cols], ref)
    print("full size: split %.3g, exact %.3g" % (e_split, e_exact))
    assert e_split <= max(2 * e_exact, 2e-6)
    plan.close()
